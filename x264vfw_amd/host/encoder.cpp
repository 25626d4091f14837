// encoder.cpp — x264_encoder_* API (boundary B1) over the MI355X hot path (boundary B3, libx264gpu.so).
//   x264_encoder_open        codec.c:1623    x264_encoder_parameters  codec.c:1630
//   x264_encoder_headers     codec.c:1650    x264_encoder_encode      codec.c:1693
//   x264_encoder_delayed_frames codec.c:1848 x264_encoder_close       codec.c:1857
// Contracts kept: NULL / negative on failure, diagnostics only through pf_log, all NALs of a
// call contiguous from nal[0].p_payload, buffers valid until the next call, param strings copied at open,
// pic_out->{i_type,b_keyframe,i_pts,i_dts} filled.  No CPU fallback: open fails without a GPU.
#include "host.hpp"
#include "dpb.hpp"
#include "batch.hpp"
#include "gopslots.hpp"
#include "quality.hpp"
#include "noisereduction.hpp"
#include "mbtreestats.hpp"
#include "ratecontrol.hpp"
#include "slicetype.hpp"
#include "settings.hpp"
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <deque>
#include <memory>
#include <string>
#include <atomic>
#include <thread>
#include <chrono>
#include <mutex>
#include <condition_variable>

using namespace x264host;

struct x264_t {
    x264_param_t param;
    std::string stat_in, stat_out;
    // host/settings.hpp: what the session really runs — the effective parameters' constants (picture structure, session mode, quantisers, profile and level, lookahead
    // window, pictures in flight).  x264_encoder_open settles them once, before anything is created; everything else reads them through `set`
    Settings settled_at_open;
    const Settings &set = settled_at_open;
    x264gpu_encoder *gpu = nullptr;
    int frame_no = 0;            // frames submitted
    int frames_since_idr = 0;
    int frame_num = 0;
    int idr_pic_id = 0;
    int sei_sent = 0;
    uint8_t *d_in = nullptr;
    x264gpu_mb *d_mb = nullptr;
    int16_t *d_lv = nullptr;
    std::vector<uint8_t> h_in;
    std::vector<x264gpu_mb> h_mb;
    std::vector<int16_t> h_lv;
    std::vector<uint8_t> out;            // bitstream of the current call
    std::vector<x264_nal_t> nals;
    std::vector<size_t> nal_off;
    SliceStats last_stats = { 0 };
    // ---- --psnr / --ssim (host/quality.hpp): the session's figures; the device result of the picture coded last (one per launch context where there are several),
    //      its host copies (two: the pipelined I / P session downloads one picture's while the one before is coded) ----
    Quality ql;
    x264gpu_quality *d_q = nullptr, hq[2] = {};
    NoiseReduction nr;                   // host/noisereduction.hpp: --nr — the session's state on the device, moved on behind every accepted picture
    MbTreeStats tstats;                  // host/mbtreestats.hpp: the macroblock-tree statistics file of a 2-pass encode (X264GPU_MBTREE_STATS=1), written or read
    const float *last_offsets = nullptr; // device: the per-macroblock quantiser offsets of the picture handed back last (x264host_last_mb_qp_offsets; nullptr: none)
    // ---- lookahead-driven decisions (threads 1 only): scenecut and CRF, both fed by x264gpu_lookahead_frame_cost ----
    x264gpu_lookahead *la = nullptr;
    int32_t *d_la = nullptr;             // device: the four sums of the last picture
    RateControl rc;                      // host/ratecontrol.hpp: which rate control the session runs, every picture's quantiser
    // ---- VBV (--vbv-maxrate / --vbv-bufsize; Settings validates them: set.vbv, set.hrd): such a session runs serially on the DPB model; a picture whose coded size would under-run the
    //      buffer is coded again at a higher quantiser (x264 re-quantises row by row while the picture is coded: the entropy coder runs behind the device here) ----
    int minigop_b = 0;                   // B pictures of the mini-GOP being coded (x264 frame->i_bframes)
    // x264host_last_vbv: the picture whose NAL units the last call returned
    struct VbvInfo { double fill_before = 0, fill_after = 0, qp_novbv = 0, qp_clipped = 0, frame_size_planned = 0, qp_final = 0; long overhead_bits = 0; int attempts = 0, filler = 0; bool valid = false; RateControl::Planned planned; } last_vbv;
    long hrd_pics_since_bp = 0;          // coded pictures since the last buffering period (cpb_removal_delay counts them, two clock ticks each)
    double t_b[5] = { 0, 0, 0, 0, 0 };          // ... sessions on the DPB model: slice-type analysis, GPU hot path, download, entropy coding, pictures
    double t_phase[6] = { 0, 0, 0, 0, 0, 0 };   // X264GPU_HOST_TIMING=1: seconds in copy-in, upload + lookahead, GPU, download, entropy coding, calls
    // ---- lookahead queue (threads 1): pictures wait here rc-lookahead deep when the macroblock-tree needs to see what follows them ----
    struct QEntry { int64_t pts; int slot; int type; int scenecut; int32_t costs[4]; x264_image_t img; int qp; int buf; bool launched; float qpm = 0.f; double qpf = 0; };      // type: 0 P, 1 I, 2 IDR; qpm: the float quantiser handed to the device (0: none), qpf: the rate control's; qp / buf / launched: set by gpu_stage
    std::deque<QEntry> queue;
    std::vector<uint8_t *> q_raw;        // device: source pictures (slot 0 is d_in when nothing is held back: zero-copy input)
    std::vector<int32_t *> q_info;       // device: lookahead block records per slot
    void *q_block[4] = { nullptr, nullptr, nullptr, nullptr };      // device: the blocks the queue's per-slot arrays are cut from (raw pictures, block records, AQ offsets, tree offsets)
    std::vector<float *> q_aq;           // device: AQ offsets per slot (x264 f_qp_offset_aq, single floats)
    float *d_tree = nullptr;             // device: macroblock-tree quantiser offsets of the picture being coded
    long la_count = 0; int la_gop = 0;   // pictures seen by the lookahead; distance from the last IDR at lookahead time
    // ---- pipelined threads-1 sessions (set.pipeline: CRF with pictures held back anyway): the GPU stage of picture n+1 runs in a helper thread while
    //      the calling thread entropy-codes picture n; every picture is handed back one call later than without it ----
    std::thread gpu_thread;
    int gpu_rc = 0;                      // result of the GPU stage in flight
    int device = 0;
    int last_qp = 0, last_scenecut = 0;  // diagnostics: quantiser and scenecut flag of the last coded picture
    float last_qpm = 0.f;                // ... and its float quantiser as the device got it (x264 rc->qpm; 0 = the integer one)
    int32_t last_costs[4] = { 0, 0, 0, 0 };
    GopSlots gops;                // host/gopslots.hpp: set.G > 1 sessions run through it alone — G closed GOPs of the stream in lock-step, dealt to the visible devices
    // set.slots_rc (X264GPU_GOP_SLOTS_RC=1, a CRF session with B pictures under --threads G): the session plans every picture as a --threads 1 session does (lookahead, slice types,
    // its own DPB model, RateControl::start — bmode_plan) and hands it to the slots instead of coding it; plan_count: pictures planned so far (coding order)
    long plan_count = 0;
    bool failed = false;                 // a GPU call failed; the session only returns errors from now on
    std::string gpu_err;                 // threads 1, pipelined: the helper thread's x264gpu_last_error() text (that buffer is thread-local)
    std::vector<x264gpu_mb> h_mb2;       // pipelined sessions: second download buffers (one picture's land while the one before is coded)
    std::vector<int16_t> h_lv2;
    // ---- sessions with B pictures (threads 1; x264 --bframes N --b-pyramid): the picture types and the coding order come from host/slicetype.hpp, the DPB, the
    //      reference lists and the slice header's share of them from host/dpb.hpp ----
    Dpb dpb;
    SliceType slicetype;                 // the display-order and coding-order queues, every picture's type
    std::vector<float *> q_tree;         // device, per queue slot: the quantiser offsets the macroblock-tree left with the picture (AQ offsets until it ran)
    // cross-session batcher (X264GPU_BATCH=N): N sessions of equal geometry and toolset share ONE device encoder with N streams; the pictures
    // they submit are coded in one lock-step launch, every session entropy-codes its own stream on its caller's thread
    Batch batch;                         // host/batch.hpp: the session's seat in its group
    // batch sessions with overlap (Batch::overlap): the picture just submitted is downloaded and entropy-coded by a helper thread while the group's next round runs;
    // its NAL units leave with the NEXT call (one picture of delay).  Two slots used in turn: the one being filled, the one waiting to be handed out
    struct Deferred { std::thread th; bool valid = false; std::atomic<bool> hurry{ false }; std::string err; std::vector<uint8_t> out; std::vector<size_t> off; std::vector<int> types; int nal_ref_idc = 0;
                      std::vector<x264gpu_mb> mb; std::vector<x264gpu_level_index> ix; std::unique_ptr<int16_t[]> lv; SliceStats stats = { 0 };      // (lv: never cleared — what is downloaded is what is read)
                      int i_type = 0, b_keyframe = 0; int64_t pts = 0, dts = 0; x264_image_t img;
                      int qp = 0, scenecut = 0; float qpm = 0.f; int32_t costs[4] = { 0, 0, 0, 0 };
                      x264gpu_quality q = {}; int q_type = 0, q_poc = 0; };      // --psnr / --ssim: the picture's statistics (downloaded with its records), slice type and POC      // the decision hooks' values of THIS picture (x264host_last_decision / _last_qpm)
    Deferred defer[2]; int defer_cur = 0;
    // ---- several pictures of ONE session in flight (threads-1 sessions on the DPB model; x264's frame threads overlap pictures too).  The b pictures of a mini-GOP, the
    //      B reference between two finished P pictures and the next P picture share only FINISHED references: each is issued through a launch context of its own (the
    //      encoder or a view of it: own scratch, the shared DPB) on a stream of its own, behind the events of the pictures it references, into a slot no picture in
    //      flight reads or writes; pictures are planned, issued and handed back in coding order, so the stream is the serial session's byte for byte ----
    struct LaunchCtx { x264gpu_encoder *gpu = nullptr; void *stream = nullptr, *ev = nullptr; x264gpu_mb *d_mb = nullptr; int16_t *d_lv = nullptr; bool busy = false; x264gpu_quality *d_q = nullptr; };
    // a picture of a session on the DPB model between plan and finish: what was decided for it, what the device is told, what the slice writer is told;
    // with several pictures in flight also its launch context and the DPB slots it reads or writes
    struct PicPlan { SliceType::Pic pl; x264gpu_pic pic; SliceParams sp; int nal_ref_idc = 0; double qpf = 0; const float *d_offsets = nullptr; bool direct_auto_write = false; char direct_char = '-';
                     const int16_t *d_mvs[2] = { nullptr, nullptr };          // the lookahead's vectors towards reference 0 of each list (nullptr: none)
                     int ctx = 0; unsigned slots_used = 0; bool last_minigop_b = false; };
    void *ev_la = nullptr;               // the default stream's position when a picture is issued: its upload, offsets and lowres vectors are complete behind it
    std::vector<LaunchCtx> lctx; std::deque<PicPlan> fl; int slot_writer[8] = { -1, -1, -1, -1, -1, -1, -1, -1 }; int last_retired_slot = -1;
    std::vector<int64_t> all_pts;        // every pts seen, in display order (the dts delay line)
    long coded_count = 0;
    // --direct temporal / auto (set.direct_mode; x264 h->stat.i_direct_score, frame->i_poc_l0ref0): the running skip-probe counts of
    // temporal [0] / spatial [1] prediction; the POC behind reference 0 of list 0 of every kept picture (INT_MIN: it had none)
    int direct_score[2] = { 0, 0 }, slot_l0ref0poc[8] = { 0 };
    char last_direct_char = '-';
};

void x264host::xlog(const x264_param_t *p, int level, const char *fmt, ...)
{
    if (!p->pf_log || level > p->i_log_level) return;
    va_list ap;
    va_start(ap, fmt);
    p->pf_log(p->p_log_private, level, fmt, ap);
    va_end(ap);
}


// threads that entropy-code row bands of ONE slice (write_slice): X264GPU_CAVLC_THREADS overrides `dflt`
static int cavlc_threads_default(int dflt)
{
    const char *e = getenv("X264GPU_CAVLC_THREADS");
    return clampi(e ? atoi(e) : dflt, 1, 64);
}

static const char kSeiText[] = "x264vfw-mi355x hot path r1 - H.264/MPEG-4 AVC codec - options: cavlc ip p8x8 i4x4 i8x8 8x8dct hex ref<=4 cqp";

static SpsParams make_sps(const x264_t *h)
{
    const x264_param_t &p = h->param;
    SpsParams s = {};
    s.profile_idc = h->set.profile_idc; s.level_idc = h->set.level_idc; s.sps_id = p.i_sps_id;
    s.mbw = h->set.mbw; s.mbh = h->set.mbh; s.crop_right = h->set.mbw * 16 - p.i_width; s.crop_bottom = h->set.mbh * 16 - p.i_height;
    s.num_ref_frames = h->param.i_frame_reference; s.log2_max_frame_num = h->set.log2_max_frame_num;
    s.sar_w = p.vui.i_sar_width; s.sar_h = p.vui.i_sar_height; s.fullrange = p.vui.b_fullrange;
    s.colorprim = p.vui.i_colorprim; s.transfer = p.vui.i_transfer; s.colmatrix = p.vui.i_colmatrix;
    s.overscan = p.vui.i_overscan; s.vidformat = p.vui.i_vidformat;
    s.num_units_in_tick = p.i_timebase_num; s.time_scale = p.i_timebase_den * 2;
    s.constraint_set0 = h->set.profile_idc == 66; s.constraint_set1 = h->set.profile_idc <= 77;
    s.mv_range = h->param.analyse.i_mv_range;
    if (h->set.dpbmode) { s.num_ref_frames = h->dpb.max_dpb; s.log2_max_poc_lsb = h->set.log2_max_poc_lsb; s.num_reorder_frames = h->dpb.num_reorder; }
    s.hrd = h->set.hrd;
    return s;
}
static PpsParams make_pps(const x264_t *h)
{
    PpsParams pp = { h->param.i_sps_id, h->param.i_sps_id, h->param.b_cabac, h->param.i_frame_reference, h->set.pic_init_qp, h->param.analyse.i_chroma_qp_offset,
                     h->param.analyse.b_transform_8x8 };
    if (h->set.bframes && h->param.analyse.b_weighted_bipred) pp.weighted_bipred_idc = 2;
    pp.weighted_pred = h->set.weightp > 0;
    return pp;
}
// access unit delimiter (--aud, 7.3.2.4, Table 7-5): primary_pic_type 0 = I slices only, 1 = I and P, 2 = I, P and B (what x264 writes for its three
// slice types); first NAL of the access unit (long start code)
static void write_aud(std::vector<uint8_t> &out, int pic_type /* 0 I, 1 P, 2 B */, bool annexb)
{
    BitWriter bw;
    bw.put((unsigned)pic_type, 3);
    bw.trailing();
    append_nal(out, 0, 9, bw.bytes(), annexb, true);
}

// appends SPS, PPS (and optionally the version SEI) to `bytes`, recording NAL offsets and types
static void write_sets(const x264_t *h, std::vector<uint8_t> &bytes, std::vector<size_t> &off, std::vector<int> &types, bool sei)
{
    const bool annexb = h->param.b_annexb != 0;
    off.push_back(bytes.size()); types.push_back(7);
    write_sps(bytes, make_sps(h), annexb);
    off.push_back(bytes.size()); types.push_back(8);
    write_pps(bytes, make_pps(h), annexb);
    if (sei) {
        off.push_back(bytes.size()); types.push_back(6);
        write_sei_version(bytes, kSeiText, annexb);
    }
}

// ---- the steps every session mode takes for a coded picture ----
// what opens the access unit of a picture of type PIC_*: the delimiter under --aud, and in front of an IDR picture (b_repeat_headers) the parameter sets, with the
// version SEI when the caller says so (sessions that write into h->out: until it has been sent once; GOP slots: in the stream's first GOP).  true: the sets were written
// Under --nal-hrd (tm: sessions with VBV on the DPB model) a keyframe also carries the buffering-period SEI behind its parameter sets, and every picture the
// picture-timing SEI in front of its slices
struct AuTiming { uint32_t initial_cpb_removal_delay, initial_cpb_removal_delay_offset, cpb_removal_delay, dpb_output_delay; };
static bool begin_access_unit(const x264_t *h, std::vector<uint8_t> &bytes, std::vector<size_t> &off, std::vector<int> &types, int pic_type, bool sei, const AuTiming *tm = nullptr)
{
    const x264_param_t &p = h->param;
    const bool annexb = p.b_annexb != 0, sets = pic_type == PIC_IDR && p.b_repeat_headers;
    if (p.b_aud) { off.push_back(bytes.size()); types.push_back(9); write_aud(bytes, pic_type <= PIC_I ? 0 : pic_type == PIC_P ? 1 : 2, annexb); }
    if (!tm) {
        if (sets) write_sets(h, bytes, off, types, sei);
        return sets;
    }
    if (sets) write_sets(h, bytes, off, types, false);
    if (pic_type == PIC_IDR) {
        off.push_back(bytes.size()); types.push_back(6);
        write_sei_buffering_period(bytes, h->set.hrd, p.i_sps_id, tm->initial_cpb_removal_delay, tm->initial_cpb_removal_delay_offset, annexb, bytes.empty());
    }
    if (sets && sei) { off.push_back(bytes.size()); types.push_back(6); write_sei_version(bytes, kSeiText, annexb); }
    off.push_back(bytes.size()); types.push_back(6);
    write_sei_pic_timing(bytes, h->set.hrd, tm->cpb_removal_delay, tm->dpb_output_delay, annexb, bytes.empty());
    return sets;
}
// the slices of the picture behind what the access unit holds so far, their NAL units tagged 5 (IDR) or 1
static void write_slices(std::vector<uint8_t> &bytes, std::vector<size_t> &off, std::vector<int> &types, const SliceParams &sp, int slices, const x264gpu_mb *mbs, const int16_t *levels,
                         bool annexb, bool idr, SliceStats *stats, int threads, const x264gpu_level_index *index = nullptr)
{
    const size_t before = off.size();
    write_picture(bytes, &off, sp, slices, mbs, levels, annexb, before == 0, stats, threads, index);
    for (size_t i = before; i < off.size(); i++) types.push_back(idr ? 5 : 1);
}
// the session-constant half of a picture's SliceParams; the caller adds what differs per picture (qp, slice_type, frame_num, idr*, nal_ref_idc, num_ref — or Dpb::fill)
static SliceParams slice_params_base(const x264_t *h)
{
    const x264_param_t &p = h->param;
    SliceParams sp = {};
    sp.mbw = h->set.mbw; sp.mbh = h->set.mbh; sp.pic_init_qp = h->set.pic_init_qp; sp.log2_max_frame_num = h->set.log2_max_frame_num; sp.log2_max_poc_lsb = h->set.log2_max_poc_lsb;
    sp.pps_id = p.i_sps_id; sp.num_ref_default = p.i_frame_reference; sp.num_ref1_default = 1;
    sp.disable_deblock_idc = p.b_deblocking_filter ? 0 : 1; sp.alpha_off_div2 = p.i_deblocking_filter_alphac0; sp.beta_off_div2 = p.i_deblocking_filter_beta;
    sp.transform8x8_mode = p.analyse.b_transform_8x8; sp.cabac = p.b_cabac; sp.slices_plain = h->set.slices_plain;
    return sp;
}
static int x264_type_of(int pic_type)
{
    return pic_type == PIC_IDR ? X264_TYPE_IDR : pic_type == PIC_I ? X264_TYPE_I : pic_type == PIC_P ? X264_TYPE_P : pic_type == PIC_BREF ? X264_TYPE_BREF : X264_TYPE_B;
}
// x264's dts of the k-th coded picture: the pts of display picture k - delay; the first `delay` ones are shifted back by the delay's duration
static int64_t coded_dts(const x264_t *h, long k)
{
    const long delay = !h->set.bframes ? 0 : h->set.bpyramid ? 2 : 1;
    const size_t np = h->all_pts.size();
    if (k >= delay) return h->all_pts[(size_t)(k - delay) < np ? (size_t)(k - delay) : np - 1];
    return h->all_pts[(size_t)k < np ? (size_t)k : np - 1] - (h->all_pts[(size_t)delay < np ? (size_t)delay : np - 1] - h->all_pts[0]);
}
static void fill_pic_out(x264_picture_t *pic_out, int i_type, bool keyframe, int64_t pts, int64_t dts, const x264_image_t *img)
{
    if (!pic_out) return;
    x264_picture_init(pic_out);
    pic_out->i_type = i_type; pic_out->b_keyframe = keyframe;
    pic_out->i_pts = pts; pic_out->i_dts = dts;
    if (img) pic_out->img = *img;
}

extern "C" {
// ---- x264_encoder_open, step by step: what the session runs is settled first (host/settings.hpp); the steps here only create what it says (each logs why it fails; a
//      failed step leaves the teardown to x264_encoder_close) ----
// the device side: the staging buffer, then the GOP slots' encoders and rings per device, or a seat in a batch group, or the session's own encoder with its launch contexts
static bool open_device(x264_t *h)
{
    x264_param_t &p = h->param;
    x264gpu_config cfg = h->set.device_config(p);
    const size_t insz = (size_t)p.i_width * p.i_height * 3 / 2;
    (void)x264gpu_get_device(&h->device);
    h->ql.open(p, h->set.G > 1);          // --psnr / --ssim: from here on h->ql.flags says whether the session computes them
    bool ok_setup = x264gpu_malloc((void **)&h->d_in, insz) == X264GPU_OK;
    if (ok_setup && h->set.G > 1) {
        // the access unit of a slot's picture (a pool thread of the unit's): AUD, the sets in front of an IDR picture (the SEI in the stream's first GOP only), the slices
        const x264_t *ch = h;
        auto write_coded = [ch](GopSlots::Coded &cd, int pic_type, long gop, SliceParams sp, const x264gpu_mb *mb, const int16_t *lv) {
            cd.bytes.clear(); cd.off.clear(); cd.types.clear();
            cd.idr = pic_type == PIC_IDR; cd.i_type = x264_type_of(pic_type);
            begin_access_unit(ch, cd.bytes, cd.off, cd.types, pic_type, gop == 0);
            sp.idr_pic_id = (int)(gop & 0xffff);
            write_slices(cd.bytes, cd.off, cd.types, sp, ch->set.slices, mb, lv, ch->param.b_annexb != 0, cd.idr, nullptr, 1);
        };
        GopSlots::Setup su = { h->set.G, h->set.keyint, h->set.nmb, h->set.qp_i, h->set.qp_p, h->set.bframes, h->set.bpyramid, h->set.weightp, h->set.log2_max_frame_num, h->set.direct_mode, h->set.dpbmode,
                               h->device, slice_params_base(h), write_coded };
        if (h->set.slots_rc) {
            // what the session's own lookahead will hand the slots with every planned picture (bmode_plan): offsets from the tree or --aq-mode 2 / 3, vectors from the
            // lookahead object the tree opens; the lookahead's wait is x264's i_slicetype_length
            su.planned = true;
            su.plan_offsets = p.rc.b_mb_tree || (p.rc.i_aq_mode >= 2 && p.rc.f_aq_strength > 0);
            su.plan_mvs = p.rc.b_mb_tree != 0;
            su.plan_wait = p.rc.b_mb_tree && h->set.lookahead_asked > h->set.bframes ? h->set.lookahead_asked : h->set.bframes;
            if (p.rc.b_mb_tree && h->set.weightp)
                xlog(&p, X264_LOG_INFO, "weightp %d in GOP slots: a fade's explicit weights are not coded (the slots of a device call share them; the lookahead still weighs fades for its costs)\n", h->set.weightp);
        }
        return h->gops.open(p, cfg, h->rc, su);
    } else if (ok_setup && h->batch.want) {
        // what the session's own lookahead will hand the group with every picture (bmode_plan): offsets from the tree or --aq-mode 2 / 3, vectors from the lookahead object
        // the tree (or a VBV plan) opens; sessions that differ in any of it, or in what shapes it, form groups of their own
        Batch::Side side;
        const bool la_object = p.rc.b_mb_tree || (h->set.vbv && h->set.lookahead_asked > 0);
        side.offsets = p.rc.b_mb_tree || (p.rc.i_aq_mode >= 2 && p.rc.f_aq_strength > 0);
        side.mvs = la_object;
        side.key = (p.rc.b_mb_tree ? 1 : 0) | p.rc.i_aq_mode << 1 | h->set.direct_mode << 4 | h->set.lookahead_asked << 8;
        ok_setup = h->batch.join(cfg, h->batch.want, insz, (size_t)h->set.nmb, h->ql.flags, p.analyse.i_noise_reduction, h->set.nr_any, side);
        if (ok_setup) xlog(&p, X264_LOG_INFO, "X264GPU_BATCH: stream %d of a batch of %d sessions%s%s\n", h->batch.index(), h->batch.size(), h->batch.queued() ? " (rounds queued: uploads overlap the device)" : "",
                           side.offsets && side.mvs ? "; the group carries each member's quantiser offsets and lookahead vectors" : side.offsets ? "; the group carries each member's quantiser offsets" :
                           side.mvs ? "; the group carries each member's lookahead vectors" : "");
        if (ok_setup && la_object && h->set.weightp)
            xlog(&p, X264_LOG_INFO, "weightp %d in a batch: a fade's explicit weights are not coded (the streams of a device call share them; the lookahead still weighs fades for its costs)\n", h->set.weightp);
    } else if (ok_setup) {
        ok_setup = x264gpu_encoder_create(&h->gpu, &cfg) == X264GPU_OK &&
                   x264gpu_malloc((void **)&h->d_mb, (size_t)h->set.nmb * sizeof(x264gpu_mb)) == X264GPU_OK &&
                   x264gpu_malloc((void **)&h->d_lv, (size_t)h->set.nmb * X264GPU_MB_LEVELS * sizeof(int16_t)) == X264GPU_OK &&
                   (!h->ql.flags || x264gpu_malloc((void **)&h->d_q, sizeof(x264gpu_quality)) == X264GPU_OK);
        ok_setup = ok_setup && h->nr.open(p, h->gpu, h->set.nr_any);
        if (ok_setup && h->set.inflight > 1) {
            h->lctx.resize((size_t)h->set.inflight);
            ok_setup = x264gpu_event_create(&h->ev_la) == X264GPU_OK;
            for (int i = 0; i < h->set.inflight && ok_setup; i++) {
                x264_t::LaunchCtx &c = h->lctx[(size_t)i];
                if (i == 0) { c.gpu = h->gpu; c.d_mb = h->d_mb; c.d_lv = h->d_lv; c.d_q = h->d_q; }
                else ok_setup = x264gpu_encoder_create_view(&c.gpu, h->gpu) == X264GPU_OK &&
                                x264gpu_malloc((void **)&c.d_mb, (size_t)h->set.nmb * sizeof(x264gpu_mb)) == X264GPU_OK &&
                                x264gpu_malloc((void **)&c.d_lv, (size_t)h->set.nmb * X264GPU_MB_LEVELS * sizeof(int16_t)) == X264GPU_OK &&
                                (!h->ql.flags || x264gpu_malloc((void **)&c.d_q, sizeof(x264gpu_quality)) == X264GPU_OK);
                ok_setup = ok_setup && x264gpu_stream_create(&c.stream) == X264GPU_OK && x264gpu_event_create(&c.ev) == X264GPU_OK;
            }
            if (ok_setup) xlog(&p, X264_LOG_INFO, "up to %d pictures of the session in flight (pictures that share only finished references; the stream is the serial one)\n", h->set.inflight);
        }
    }
    if (!ok_setup) {
        xlog(&p, X264_LOG_ERROR, "GPU encoder setup failed: %s\n", x264gpu_last_error());
        return false;
    }
    return true;
}

// lookahead and slice-type objects, the queue's device ring
static bool open_lookahead(x264_t *h)
{
    x264_param_t &p = h->param;
    const size_t insz = (size_t)p.i_width * p.i_height * 3 / 2;
    if (h->set.lookahead) {
        if (x264gpu_lookahead_create(&h->la, p.i_width, p.i_height, 1, p.analyse.i_me_range, p.analyse.i_subpel_refine) != X264GPU_OK ||
            x264gpu_malloc((void **)&h->d_la, 4 * sizeof(int32_t)) != X264GPU_OK) {
            xlog(&p, X264_LOG_ERROR, "GPU lookahead setup failed: %s\n", x264gpu_last_error());
            return false;
        }
    }
    h->set.log_lookahead(p);
    h->q_raw.assign((size_t)h->set.Q, nullptr); h->q_info.assign((size_t)h->set.Q, nullptr); h->q_aq.assign((size_t)h->set.Q, nullptr); h->q_tree.assign((size_t)h->set.Q, nullptr);
    if (h->set.dpbmode && !h->slicetype.open(p, h->rc, { h->set.Q, h->set.st_wait, h->set.mbw, h->set.mbh, h->set.bframes, h->set.bpyramid, h->set.weightp, h->set.mbtree, h->set.vbv, h->set.aq_strength, h->set.tree_strength,
                                                     h->q_raw.data(), h->q_aq.data(), h->q_tree.data() })) return false;
    if (h->set.Q == 1) h->q_raw[0] = h->d_in;            // no delay: the staging buffer is the one slot; with a delay the ring is separate,
                                                     // because a zero-copy caller rewrites the staging buffer every call
    {
        // one device block per array, cut into the queue's slots (an allocation and a release each cost a fraction of a millisecond: thousands of sessions open and close)
        bool ok = true;
        const size_t Q = (size_t)h->set.Q, insz_al = (insz + 255) & ~(size_t)255, nmbf = ((size_t)h->set.nmb * sizeof(float) + 255) & ~(size_t)255, ninfo = ((size_t)h->set.nmb * 4 * sizeof(int32_t) + 255) & ~(size_t)255;
        const bool want_aq = h->set.mbtree || h->slicetype.aq_costs || h->set.aq_mode >= 2 || h->tstats.reading, want_tree = (h->set.mbtree && h->set.dpbmode) || h->tstats.reading;
        if (!h->q_raw[0]) ok = x264gpu_malloc((void **)&h->q_block[0], Q * insz_al) == X264GPU_OK;
        if (ok && h->set.mbtree) ok = x264gpu_malloc((void **)&h->q_block[1], Q * ninfo) == X264GPU_OK;
        if (ok && want_aq) ok = x264gpu_malloc((void **)&h->q_block[2], Q * nmbf) == X264GPU_OK;
        if (ok && want_tree) ok = x264gpu_malloc((void **)&h->q_block[3], Q * nmbf) == X264GPU_OK;
        for (size_t i = 0; i < Q && ok; i++) {
            if (!h->q_raw[i]) h->q_raw[i] = (uint8_t *)h->q_block[0] + i * insz_al;
            if (h->set.mbtree) h->q_info[i] = (int32_t *)((uint8_t *)h->q_block[1] + i * ninfo);
            if (want_aq) h->q_aq[i] = (float *)((uint8_t *)h->q_block[2] + i * nmbf);
            if (want_tree) h->q_tree[i] = (float *)((uint8_t *)h->q_block[3] + i * nmbf);
        }
        if (ok && h->set.mbtree) ok = x264gpu_malloc((void **)&h->d_tree, (size_t)h->set.nmb * sizeof(float)) == X264GPU_OK;
        if (!ok) {
            xlog(&p, X264_LOG_ERROR, "GPU lookahead queue setup failed: %s\n", x264gpu_last_error());
            return false;
        }
    }
    return true;
}

// host buffers
static void open_host_buffers(x264_t *h)
{
    x264_param_t &p = h->param;
    const size_t insz = (size_t)p.i_width * p.i_height * 3 / 2;
    h->h_in.resize(insz);
    // (a batch session whose pictures are downloaded and coded by its helper threads keeps the records in the two deferred slots instead: 7 MB less to clear per open)
    // (... and GOP slots own their download buffers)
    if (!h->batch.overlap() && h->set.G == 1) { h->h_mb.resize((size_t)h->set.nmb); h->h_lv.resize((size_t)h->set.nmb * X264GPU_MB_LEVELS); }
    if (h->set.pipeline) { h->h_mb2.resize(h->h_mb.size()); h->h_lv2.resize(h->h_lv.size()); }
}

x264_t *x264_encoder_open(x264_param_t *param)
{
    if (!param) return nullptr;
    if (param->i_width < 16 || param->i_height < 16 || (param->i_width & 1) || (param->i_height & 1)) {
        xlog(param, X264_LOG_ERROR, "invalid width x height (%dx%d)\n", param->i_width, param->i_height);
        return nullptr;
    }
    if ((param->i_csp & X264_CSP_MASK) != X264_CSP_I420) { xlog(param, X264_LOG_ERROR, "only i420 input is supported\n"); return nullptr; }
    if (x264gpu_device_count() < 1) { xlog(param, X264_LOG_ERROR, "no MI355X device visible (there is no CPU fallback)\n"); return nullptr; }
    x264_t *h = new x264_t();
    h->param = *param;
    x264_param_t &p = h->param;
    if (p.rc.psz_stat_in) { h->stat_in = p.rc.psz_stat_in; p.rc.psz_stat_in = &h->stat_in[0]; }     // codec.c:1386 stack buffers
    if (p.rc.psz_stat_out) { h->stat_out = p.rc.psz_stat_out; p.rc.psz_stat_out = &h->stat_out[0]; }
    h->settled_at_open.settle(p, h->rc, h->dpb, h->tstats, h->batch.want);
    if (!open_device(h) || !open_lookahead(h) || !h->rc.open(p, h->set.mbw, h->set.mbh, h->set.bframes, h->set.qp_i, h->set.qp_p) ||
        !h->tstats.open(p, p.rc.psz_stat_in, p.rc.psz_stat_out, h->set.nmb)) { x264_encoder_close(h); return nullptr; }
    if (h->tstats.reading) p.rc.b_mb_tree = 1;          // reported back: the second pass codes with the first pass' tree (every reader of the flag has run)
    open_host_buffers(h);
    xlog(&p, X264_LOG_INFO, "MI355X hot path: %dx%d, %d MBs, CQP I:%d P:%d, keyint %d, level %d\n", p.i_width, p.i_height, h->set.nmb,
         h->set.qp_i, h->set.qp_p, h->set.keyint, h->set.level_idc);
    return h;
}

void x264_encoder_parameters(x264_t *h, x264_param_t *param)
{
    if (!h || !param) return;
    *param = h->param;
    if (h->set.slices > 1 && !h->set.slices_plain && h->set.G <= 1) param->i_threads = h->set.slices;      // slice threads: i_threads is the slice count, as in x264
}

static void publish_nals(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, const std::vector<int> &types)
{
    h->nals.resize(h->nal_off.size());
    for (size_t i = 0; i < h->nal_off.size(); i++) {
        x264_nal_t &n = h->nals[i];
        memset(&n, 0, sizeof(n));
        size_t end = i + 1 < h->nal_off.size() ? h->nal_off[i + 1] : h->out.size();
        n.p_payload = h->out.data() + h->nal_off[i];
        n.i_payload = (int)(end - h->nal_off[i]);
        n.i_type = types[i];
        n.i_ref_idc = types[i] == 6 ? 0 : types[i] == 1 ? 2 : 3;
        n.b_long_startcode = 1;
    }
    *pp_nal = h->nals.data();
    *pi_nal = (int)h->nals.size();
}

int x264_encoder_headers(x264_t *h, x264_nal_t **pp_nal, int *pi_nal)
{
    if (!h || !pp_nal || !pi_nal) return -1;
    h->out.clear(); h->nal_off.clear();
    std::vector<int> types;
    write_sets(h, h->out, h->nal_off, types, true);               // nal[0]=SPS nal[1]=PPS nal[2]=SEI (output/raw.c:41-47)
    publish_nals(h, pp_nal, pi_nal, types);
    return (int)h->out.size();
}

static int gop_slots_pop(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out);
// ---- --threads G > 1 (host/gopslots.hpp): the picture goes to the slots, or the input has ended; then the next coded picture in output order, if there is one ----
static int encode_gop_slots(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_in, x264_picture_t *pic_out, bool resident)
{
    GopSlots &gs = h->gops;
    const int rc = pic_in ? gs.put({ h->h_in.data(), h->d_in, resident, h->la, h->d_la }, pic_in->i_pts) : gs.flush();
    h->failed |= gs.failed;
    if (rc < 0) return -1;
    if (pic_in && gs.with_b()) h->all_pts.push_back(pic_in->i_pts);
    return gop_slots_pop(h, pp_nal, pi_nal, pic_out);
}
static int gop_slots_pop(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out)
{
    GopSlots &gs = h->gops;
    GopSlots::Coded c;
    if (!gs.pop(c)) return 0;
    h->out = std::move(c.bytes);
    h->nal_off = c.off;
    publish_nals(h, pp_nal, pi_nal, c.types);
    if (gs.with_b()) {
        for (size_t i = 0; i < h->nals.size(); i++) if (c.types[i] == 1 || c.types[i] == 5) h->nals[i].i_ref_idc = c.ref_idc;
        // coding order: the picture's own pts (its display place in its GOP) and x264's dts
        const long k = c.index, gop_base = k - k % h->set.keyint;
        const size_t np = h->all_pts.size(), di = (size_t)(gop_base + c.disp);
        fill_pic_out(pic_out, c.i_type, c.idr, h->all_pts[di < np ? di : np - 1], coded_dts(h, k), nullptr);
    } else fill_pic_out(pic_out, c.idr ? X264_TYPE_IDR : X264_TYPE_P, c.idr, c.pts, c.pts, nullptr);
    h->frame_no++;
    return (int)h->out.size();
}

// GPU stage of queue[idx]: macroblock-tree over the pictures queued behind it (up to the next intra picture), rate control, the hot
// path and the download of its records / levels into host buffer pair `buf` — in a helper thread when `async` (join_gpu waits).
static void join_gpu(x264_t *h) { if (h->gpu_thread.joinable()) h->gpu_thread.join(); }

static int gpu_stage(x264_t *h, size_t idx, int buf, bool async)
{
    const x264_param_t &p = h->param;
    x264_t::QEntry &e = h->queue[idx];
    const bool idr = e.type == 2, intra_pic = e.type == 1;
    if (h->set.mbtree) {
        // macroblock_tree: this picture and the P pictures behind it that (transitively) reference it; an intra picture ends the chain
        const int32_t *info[256]; const float *aq[256];
        int n = 0;
        for (size_t j = idx; j < h->queue.size(); j++) {
            const x264_t::QEntry &q = h->queue[j];
            if (n > 0 && q.type != 0) break;
            info[n] = h->q_info[(size_t)q.slot]; aq[n] = h->q_aq[(size_t)q.slot];
            if (++n == 256) break;
        }
        if (x264gpu_lookahead_mbtree(h->la, info, h->set.aq_strength != 0.f ? aq : nullptr, n, h->set.tree_strength, h->d_tree, nullptr) != X264GPU_OK ||
            x264gpu_encoder_set_mb_qp_offsets(h->gpu, h->d_tree) != X264GPU_OK) {
            xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: macroblock-tree failed: %s\n", x264gpu_last_error());
            return -1;
        }
    }
    // (pictures leave in the order they came: the rate control's count of them is the display index)
    const int qp_now = h->rc.start(idr ? PIC_IDR : intra_pic ? PIC_I : PIC_P, h->rc.frames_done, e.costs, nullptr, &e.qpf);
    if (h->rc.by_cost()) {
        // x264_ratecontrol_mb_qp adds the AQ / macroblock-tree offsets to the FLOAT quantiser (rc->qpm) before the one rounding
        e.qpm = near_qpm(e.qpf, qp_now);
        if (x264gpu_encoder_set_qp(h->gpu, qp_now, qp_now) != X264GPU_OK || x264gpu_encoder_set_qpm(h->gpu, e.qpm) != X264GPU_OK) return -1;
    } else if (!h->rc.zones.empty() && x264gpu_encoder_set_qp(h->gpu, qp_now, qp_now) != X264GPU_OK) return -1;          // (constant quantiser: only zones move what the device has)
    e.qp = qp_now; e.buf = buf; e.launched = true;
    const int st = idr ? X264GPU_SLICE_I : intra_pic ? X264GPU_SLICE_I_NONIDR : X264GPU_SLICE_P;
    const uint8_t *src = h->q_raw[(size_t)e.slot];
    x264gpu_mb *hmb = buf ? h->h_mb2.data() : h->h_mb.data();
    int16_t *hlv = buf ? h->h_lv2.data() : h->h_lv.data();
    x264gpu_quality *hq = &h->hq[buf];
    auto run = [h, src, st, hmb, hlv, hq]() {
        h->gpu_rc = x264gpu_encode_frames(h->gpu, src, st, h->d_mb, h->d_lv, nullptr) != X264GPU_OK ||
                    (h->ql.flags && (h->ql.queue(h->gpu, h->d_q, nullptr) != X264GPU_OK || x264gpu_memcpy_d2h(hq, h->d_q, sizeof(*hq), nullptr) != X264GPU_OK)) ||
                    x264gpu_memcpy_d2h(hmb, h->d_mb, h->h_mb.size() * sizeof(x264gpu_mb), nullptr) != X264GPU_OK ||
                    x264gpu_memcpy_d2h(hlv, h->d_lv, h->h_lv.size() * sizeof(int16_t), nullptr) != X264GPU_OK ? -1 : 0;
        if (h->gpu_rc) h->gpu_err = x264gpu_last_error();          // the error text lives in this thread's buffer: keep it for the caller's log
    };
    if (async) h->gpu_thread = std::thread([h, run]() { x264gpu_set_device(h->device); run(); });
    else run();
    return 0;
}

// Hands back the oldest picture of the lookahead queue: its GPU stage (unless a helper thread already ran it), then headers + entropy
// coding.  Returns the bytes of its NAL units, 0 when the pipelined session only started a picture.
static int encode_queued(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out, bool flushing)
{
    const x264_param_t &p = h->param;
    if (!h->queue.front().launched) {
        if (gpu_stage(h, 0, 0, h->set.pipeline) < 0) return -1;
        if (h->set.pipeline && !flushing) return 0;              // its results are collected by the next call
    }
    join_gpu(h);
    if (h->gpu_rc) { xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: GPU hot path failed: %s\n", h->gpu_err.c_str()); return -1; }
    // pipelined: the next picture has its whole lookahead window (or the input has ended): start its GPU stage behind this one's coding
    if (h->set.pipeline && h->queue.size() >= 2 && (flushing || (int)h->queue.size() >= h->set.L + 2) &&
        gpu_stage(h, 1, h->queue.front().buf ^ 1, true) < 0) return -1;
    const x264_t::QEntry e = h->queue.front();
    const bool idr = e.type == 2, intra_pic = e.type == 1;
    const int qp_now = e.qp;
    const int st = idr ? X264GPU_SLICE_I : intra_pic ? X264GPU_SLICE_I_NONIDR : X264GPU_SLICE_P;
    const x264gpu_mb *hmb = e.buf ? h->h_mb2.data() : h->h_mb.data();
    const int16_t *hlv = e.buf ? h->h_lv2.data() : h->h_lv.data();
    h->last_scenecut = e.scenecut; h->last_qp = qp_now; h->last_qpm = e.qpm;
    memcpy(h->last_costs, e.costs, sizeof(e.costs));
    if (idr) { h->frames_since_idr = 0; h->frame_num = 0; }
    // ---- host: headers + entropy coding ----
    const int type = idr ? PIC_IDR : intra_pic ? PIC_I : PIC_P;
    h->out.clear(); h->nal_off.clear();
    std::vector<int> types;
    if (begin_access_unit(h, h->out, h->nal_off, types, type, !h->sei_sent)) h->sei_sent = 1;
    SliceParams sp = slice_params_base(h);
    sp.slice_type = st == X264GPU_SLICE_P ? X264GPU_SLICE_P : X264GPU_SLICE_I; sp.qp = qp_now; sp.frame_num = h->frame_num;
    sp.idr = idr; sp.idr_pic_id = h->idr_pic_id; sp.nal_ref_idc = idr ? 3 : 2;
    sp.num_ref = h->frames_since_idr < p.i_frame_reference ? (h->frames_since_idr > 0 ? h->frames_since_idr : 1) : p.i_frame_reference;
    h->last_stats.skip = 0;
    write_slices(h->out, h->nal_off, types, sp, h->set.slices, hmb, hlv, p.b_annexb != 0, idr, &h->last_stats, h->set.cavlc_threads);
    publish_nals(h, pp_nal, pi_nal, types);
    if (const char *dd = getenv("X264GPU_DUMP_RECORDS")) {          // debugging aid, in the layout of encode_bmode's dump: a picture description (slice type and quantiser alone), records, levels, zero offsets
        char fn[512];
        snprintf(fn, sizeof(fn), "%s/pic%04ld.bin", dd, (long)h->frame_no);
        if (FILE *fp = fopen(fn, "wb")) {
            x264gpu_pic dp = {};
            dp.slice_type = st; dp.qp = qp_now;
            const std::vector<float> off((size_t)h->set.nmb, 0.f);
            fwrite(&dp, sizeof(dp), 1, fp);
            fwrite(hmb, sizeof(x264gpu_mb), (size_t)h->set.nmb, fp);
            fwrite(hlv, sizeof(int16_t), (size_t)h->set.nmb * X264GPU_MB_LEVELS, fp);
            fwrite(off.data(), sizeof(float), off.size(), fp);
            fclose(fp);
        }
    }
    fill_pic_out(pic_out, x264_type_of(type), idr, e.pts, e.pts, &e.img);
    if (h->ql.flags) h->ql.frame_end(p, h->hq[e.buf], st == X264GPU_SLICE_P ? 1 : 0, mean_mb_qp(hmb, (size_t)h->set.nmb), 2 * h->frames_since_idr, h->out.size());
    if (idr) h->idr_pic_id = (h->idr_pic_id + 1) & 0xffff;
    h->frame_num = (h->frame_num + 1) & ((1 << h->set.log2_max_frame_num) - 1);
    h->rc.end(h->out.size(), type, h->frame_no, e.qpf);          // (no statistics file off the DPB model)
    h->frames_since_idr++;
    h->frame_no++;
    h->queue.pop_front();
    return (int)h->out.size();
}


// --nal-hrd: the delays a picture's SEI messages carry, from the buffer's state in front of it (Annex C: removal times are cpb_removal_delay clock ticks behind
// the last buffering-period picture's, two ticks a picture; a picture is output dpb_output_delay ticks after its removal, which puts the output times in display
// order two ticks apart: 2 x (display index - coding index + the reorder depth))
static bool au_timing(const x264_t *h, const SliceType::Pic &pl, AuTiming &tm)
{
    if (!h->set.hrd.present) return false;
    const double rate = h->set.hrd.bit_rate_unscaled, size = h->set.hrd.cpb_size_unscaled;
    const double fill = h->rc.buffer_fill_final < 0 ? 0 : h->rc.buffer_fill_final > size ? size : h->rc.buffer_fill_final;
    tm.initial_cpb_removal_delay = (uint32_t)floor(90000.0 * fill / rate);
    tm.initial_cpb_removal_delay_offset = (uint32_t)floor(90000.0 * size / rate) - tm.initial_cpb_removal_delay;
    tm.cpb_removal_delay = (uint32_t)(2 * h->hrd_pics_since_bp);
    const long delay = 2 * ((long)pl.e.frame - h->coded_count + h->dpb.num_reorder);
    tm.dpb_output_delay = (uint32_t)(delay > 0 ? delay : 0);
    return true;
}
// the bits of the NAL units a picture's access unit opens with (VBV: x264_ratecontrol_start's overhead)
static long au_overhead_bits(const x264_t *h, const SliceType::Pic &pl)
{
    std::vector<uint8_t> bytes; std::vector<size_t> off; std::vector<int> types;
    AuTiming tm;
    const bool timed = au_timing(h, pl, tm);
    begin_access_unit(h, bytes, off, types, pl.type, !h->sei_sent, timed ? &tm : nullptr);
    return (long)bytes.size() * 8;
}

// ---- the picture path of sessions on the DPB model: plan, launch, finish --------------------------------------------------------------
// One picture a call (encode_bmode), its batched variant whose pictures leave a call later (bmode_defer) and several pictures in flight (inflight_issue /
// inflight_retire) are built from the same three steps; what they do differently is an argument or a branch here, each with the mode that needs it.

// plan: takes the next picture of the coding order and settles everything the device and the slice writer will be told — the DPB model's plan (the follow list
// counts from coded_index, the picture's place in the coding order: pictures in flight have not been counted yet), the quantiser, the direct mode, the lookahead's
// vectors and the quantiser offsets on `gpu` (the encoder that will run it: the session's, or a launch context's), what later pictures' rate control and direct
// mode read of it by DPB slot, the slice parameters.  Dpb::commit stays with the caller (serial: after the slices, deferred: before the helper thread starts,
// in flight: when the picture is issued).  serial: one picture at a time, so --direct auto can follow the skip counts of the picture before
static void bmode_plan(x264_t *h, x264_t::PicPlan &f, x264gpu_encoder *gpu, long coded_index, bool serial)
{
    f.pl = h->slicetype.pop();
    const SliceType::Pic &pl = f.pl;
    const std::deque<SliceType::Pic> &behind = h->slicetype.queue();
    // the disposable pictures coded right behind this one (x264_reference_hierarchy_reset looks at them)
    int fc[16], ff[16], nf = 0;
    for (size_t i = 0; i < behind.size() && nf < 16 && behind[i].type == PIC_B; i++) { fc[nf] = (int)(coded_index + 1 + (long)i); ff[nf] = behind[i].e.frame; nf++; }
    // (the explicit weights of a picture are the same in every stream of a device call: a member of a batch group, whose lookahead would find its own, codes fades unweighted)
    // (... and so does a session whose pictures are coded by GOP slots)
    const DpbPlan plan = h->dpb.plan(pl.type, pl.e.frame, nf, fc, ff, pl.type == PIC_P && pl.e.w.on && !h->batch.joined() && !h->set.slots_rc ? &pl.e.w : nullptr);
    f.nal_ref_idc = plan.nal_ref_idc;
    x264gpu_pic &pic = f.pic;
    pic = plan.pic;
    const RateControl::BRefs near = { { pic.slot[0][0], pic.slot[1][0] }, { abs(pic.poc - plan.list_poc[0][0]), abs(pic.poc - plan.list_poc[1][0]) } };      // (read for a B picture)
    const bool is_b = pl.type == PIC_B || pl.type == PIC_BREF;
    if (h->set.vbv) {
        // x264 frame->i_bframes / b_last_minigop_bframe (every picture of a mini-GOP knows how many B pictures it holds), and the header NAL units the
        // access unit opens with (x264_ratecontrol_start's overhead)
        if (!is_b) h->minigop_b = (int)behind.size();          // (what is left of the mini-GOP in the coding queue: its B pictures)
        f.last_minigop_b = is_b && behind.empty();
        h->rc.vbv_picture(&pl.e.planned, h->minigop_b, f.last_minigop_b, au_overhead_bits(h, pl));
    }
    pic.qp = h->rc.start(pl.type, pl.e.frame, pl.e.costs, &near, &f.qpf);
    if (h->set.vbv) {
        x264_t::VbvInfo &v = h->last_vbv;
        v.valid = true; v.fill_before = h->rc.buffer_fill; v.qp_novbv = h->rc.qp_novbv; v.qp_clipped = f.qpf; v.frame_size_planned = h->rc.frame_size_planned;
        v.planned = pl.e.planned; v.attempts = 1; v.filler = 0; v.overhead_bits = au_overhead_bits(h, pl);
    }
    // x264_ratecontrol_mb_qp: a macroblock's quantiser is round(rc->qpm + its AQ / macroblock-tree offset) with qpm the picture's FLOAT quantiser
    pic.qpm = near_qpm(f.qpf, pic.qp);
    f.direct_auto_write = false;
    if (is_b && h->set.direct_mode != 1) {
        // x264 slice_header_init: temporal direct prediction is considered only when the co-located picture's reference 0 is this picture's reference 0;
        // --direct auto (serial only: sessions with pictures in flight never run it): the mode whose skip probe passed more often so far
        // (h->stat.i_direct_score), every macroblock probing both again
        bool spatial = true;
        if (pic.nref[0] && pic.nref[1] && h->slot_l0ref0poc[pic.slot[1][0]] == plan.list_poc[0][0]) {
            f.direct_auto_write = serial && h->set.direct_mode == 3;
            spatial = f.direct_auto_write ? h->direct_score[1] > h->direct_score[0] : false;
        }
        pic.direct_temporal = !spatial; pic.direct_auto = f.direct_auto_write;
        h->dpb.set_direct(pic.direct_temporal, pic.direct_auto);
    }
    if (h->slicetype.analyses()) {
        // x264_mb_predict_mv_ref16x16: the lookahead's vectors towards reference 0 of each list as search candidates, when that search ran
        const int dist0 = pic.nref[0] ? (pic.poc - plan.list_poc[0][0]) / 2 : 0, dist1 = pic.nref[1] ? (plan.list_poc[1][0] - pic.poc) / 2 : 0;
        f.d_mvs[0] = h->slicetype.lowres_mvs(pl.e.slot, 0, dist0); f.d_mvs[1] = h->slicetype.lowres_mvs(pl.e.slot, 1, dist1);
        if (gpu) { x264gpu_encoder_set_lowres_mvs(gpu, f.d_mvs[0]); x264gpu_encoder_set_lowres_mvs1(gpu, f.d_mvs[1]); }
    }
    f.d_offsets = nullptr;
    if (h->slicetype.analyses() && h->set.mbtree)          // P / I / B-reference pictures: what the tree left (AQ - tree); other B pictures: the AQ offsets alone (x264 f_qp_offset_aq)
        f.d_offsets = pl.type == PIC_B ? h->q_aq[(size_t)pl.e.slot] : h->q_tree[(size_t)pl.e.slot];
    else if (h->tstats.reading) {
        // a second pass over the macroblock-tree statistics file: a kept picture's record, unpacked into its slot; every other picture the AQ offsets alone
        const int got = h->tstats.read_record(h->param, coded_index, pl.type, h->q_tree[(size_t)pl.e.slot], nullptr);
        if (got < 0) h->failed = true;
        f.d_offsets = got > 0 ? h->q_tree[(size_t)pl.e.slot] : h->set.aq_strength != 0.f ? h->q_aq[(size_t)pl.e.slot] : nullptr;
    }
    else if (h->set.aq_mode >= 2 && h->set.aq_strength != 0.f) f.d_offsets = h->q_aq[(size_t)pl.e.slot];      // --aq-mode 2 / 3: the offsets computed when the picture arrived
    // (the serial path names a buffer only when there is one; a launch context is always told, "none" included — and so is a second pass over the tree file,
    //  whose pictures take turns between two kinds of offsets or none).  A member of a batch group has no encoder of its own (gpu == nullptr): its vectors and offsets go
    //  to the group with the picture (Batch::submit), which tells the group's encoder for all streams at once
    if (gpu && (f.d_offsets || !serial || h->tstats.reading)) x264gpu_encoder_set_mb_qp_offsets(gpu, f.d_offsets);
    if (plan.nal_ref_idc) h->rc.kept(pic.dst, f.qpf, pl.type);
    if (plan.nal_ref_idc) h->slot_l0ref0poc[pic.dst] = pic.nref[0] ? plan.list_poc[0][0] : INT_MIN;
    f.direct_char = is_b ? (pic.direct_temporal ? 't' : 's') : '-';
    f.sp = slice_params_base(h);
    f.sp.qp = pic.qp;
    h->dpb.fill(f.sp);
}

// finish, on the caller's thread: the picture becomes the one the diagnostics hooks describe, its access unit is opened in h->out (AUD, sets in front of an IDR
// picture).  idr_pic_id is read here — when the picture is handed to the slice writer, which for a picture in flight is when it retires, not when it was planned
static bool bmode_open_au(x264_t *h, x264_t::PicPlan &f, std::vector<int> &types)
{
    const SliceType::Pic &pl = f.pl;
    h->last_direct_char = f.direct_char;
    h->last_scenecut = pl.e.scenecut; h->last_qp = f.pic.qp; h->last_qpm = f.pic.qpm; h->last_offsets = f.d_offsets;
    memcpy(h->last_costs, pl.e.costs, sizeof(pl.e.costs));
    h->out.clear(); h->nal_off.clear();
    AuTiming tm;
    const bool timed = au_timing(h, pl, tm);
    const bool sets = begin_access_unit(h, h->out, h->nal_off, types, pl.type, !h->sei_sent, timed ? &tm : nullptr);          // (true: the caller marks the version SEI sent once the access unit is final)
    f.sp.idr_pic_id = h->idr_pic_id;
    return sets;
}
// ... and the session's counters move past it
static void bmode_count(x264_t *h, bool idr)
{
    h->t_b[4] += 1;
    if (idr) h->idr_pic_id = (h->idr_pic_id + 1) & 0xffff;
    h->coded_count++;
    h->frame_no++;
}

// finish: the picture's NAL units from its downloaded records, pic_out, what the rate control learns from its size (x264_ratecontrol_end: 2-pass and ABR sessions,
// which always run serially), the counters; returns the bytes of the NAL units
static int quality_type(int pic_type) { return pic_type == PIC_IDR || pic_type == PIC_I ? 0 : pic_type == PIC_P ? 1 : 2; }
// finish, first half: the access unit in h->out — what opens it, then the picture's slices from its downloaded records.  May run again for the same picture (a VBV
// session codes a picture again when it does not fit): nothing of the session moves here.  true: the parameter sets were written
static bool bmode_write_au(x264_t *h, x264_t::PicPlan &f, std::vector<int> &types, const x264gpu_mb *mbs, const int16_t *levels)
{
    types.clear();
    const bool sets = bmode_open_au(h, f, types);
    h->last_stats.skip = 0;
    write_slices(h->out, h->nal_off, types, f.sp, h->set.slices, mbs, levels, h->param.b_annexb != 0, f.pl.type == PIC_IDR, &h->last_stats, h->set.cavlc_threads);
    return sets;
}
// ... second half: the written access unit is the picture's
static int bmode_finish_written(x264_t *h, x264_t::PicPlan &f, std::vector<int> &types, bool sets, const x264gpu_mb *mbs, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out)
{
    const x264_param_t &p = h->param;
    const SliceType::Pic &pl = f.pl;
    const bool idr = pl.type == PIC_IDR;
    if (sets) h->sei_sent = 1;
    // x264_ratecontrol_end; a session that writes statistics or follows a plan is told what the picture's macroblocks were
    RateControl::PicStats ps;
    if (h->rc.pass1 || h->rc.pass2) {
        for (size_t i = 0; i < (size_t)h->set.nmb; i++) {
            const x264gpu_mb &m = mbs[i];
            if (m.type <= X264GPU_MB_I16x16) ps.imb++; else if (m.type == X264GPU_MB_P_SKIP || m.type == X264GPU_MB_B_SKIP) ps.smb++; else ps.pmb++;
        }
        ps.aq_mean = mean_mb_qp(mbs, (size_t)h->set.nmb); ps.mv_bits = h->last_stats.mv_bits; ps.tex_bits = h->last_stats.tex_bits; ps.direct = h->last_direct_char;
    }
    const int filler = h->rc.end(h->out.size(), pl.type, pl.e.frame, f.qpf, &ps);
    if (filler > 0) { h->nal_off.push_back(h->out.size()); types.push_back(12); write_filler(h->out, filler - h->rc.filler_overhead(), p.b_annexb != 0); }          // --nal-hrd cbr: what the buffer cannot hold
    if (h->set.vbv) { h->last_vbv.fill_after = h->rc.buffer_fill_final; h->last_vbv.filler = filler; h->last_vbv.qp_final = f.qpf; h->hrd_pics_since_bp = idr ? 1 : h->hrd_pics_since_bp + 1; }
    publish_nals(h, pp_nal, pi_nal, types);
    for (size_t i = 0; i < h->nals.size(); i++) if (types[i] == 1 || types[i] == 5) h->nals[i].i_ref_idc = f.nal_ref_idc;
    fill_pic_out(pic_out, x264_type_of(pl.type), idr, pl.e.pts, coded_dts(h, h->coded_count), &pl.e.img);
    if (h->ql.flags) h->ql.frame_end(p, h->hq[0], quality_type(pl.type), mean_mb_qp(mbs, (size_t)h->set.nmb), f.pic.poc, h->out.size());          // (h->hq[0]: downloaded with the records)
    bmode_count(h, idr);
    return (int)h->out.size();
}
static int bmode_finish(x264_t *h, x264_t::PicPlan &f, const x264gpu_mb *mbs, const int16_t *levels, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out)
{
    std::vector<int> types;
    const bool sets = bmode_write_au(h, f, types, mbs, levels);
    return bmode_finish_written(h, f, types, sets, mbs, pp_nal, pi_nal, pic_out);
}

// a helper thread still at work is told to hurry (it may be waiting for the group's next round), its sleep ended, and joined
static void join_deferred(x264_t *h, x264_t::Deferred &d)
{
    if (!d.th.joinable()) return;
    d.hurry = true;
    h->batch.wake();
    d.th.join();
}

// hands out a picture a helper thread finished (batch sessions with overlap): waits for the thread, publishes its NAL units; 0 when the slot is empty
static int publish_deferred(x264_t *h, x264_t::Deferred &d, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out)
{
    if (!d.valid) return 0;
    h->batch.timed(Batch::JOIN, 0, [&] { join_deferred(h, d); });
    d.valid = false;
    if (!d.err.empty()) { xlog(&h->param, X264_LOG_ERROR, "x264_encoder_encode: download of a batched picture failed: %s\n", d.err.c_str()); h->failed = true; return -1; }
    h->out.swap(d.out); h->nal_off = d.off; h->last_stats = d.stats;
    // the diagnostics hooks describe the picture whose NAL units this call returns, not the one submitted meanwhile
    h->last_qp = d.qp; h->last_qpm = d.qpm; h->last_scenecut = d.scenecut; memcpy(h->last_costs, d.costs, sizeof(d.costs));
    publish_nals(h, pp_nal, pi_nal, d.types);
    for (size_t i = 0; i < h->nals.size(); i++) if (d.types[i] == 1 || d.types[i] == 5) h->nals[i].i_ref_idc = d.nal_ref_idc;
    fill_pic_out(pic_out, d.i_type, d.b_keyframe, d.pts, d.dts, &d.img);
    if (h->ql.flags) h->ql.frame_end(h->param, d.q, d.q_type, mean_mb_qp(d.mb.data(), d.mb.size()), d.q_poc, h->out.size());
    return (int)h->out.size();
}

// finish of a batch session with overlap: everything the slice writer needs is fixed, so a helper thread downloads this stream's records and levels (round's buffer
// pair `bbuf`, on the group's download stream) and writes the slices behind the header NAL units while the group's next round runs; the DPB moves on at once (the
// next picture's plan needs it) and the NAL units leave with the NEXT call: returns the picture of the call before (0: none yet).
// (No x264_ratecontrol_end and no statistics line here: x264_encoder_open admits constant-quantiser and CRF sessions into a batch only.)
static int bmode_defer(x264_t *h, x264_t::PicPlan &f, int bbuf, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out)
{
    const x264_param_t &p = h->param;
    const SliceType::Pic &pl = f.pl;
    const bool idr = pl.type == PIC_IDR;
    std::vector<int> types;
    if (bmode_open_au(h, f, types)) h->sei_sent = 1;
    x264_t::Deferred &d = h->defer[h->defer_cur];
    if (d.th.joinable()) d.th.join();          // (handed out two calls ago: long finished)
    d.out = h->out; d.off = h->nal_off; d.types = types; d.err.clear(); d.nal_ref_idc = f.nal_ref_idc; d.stats = SliceStats{ 0 };
    d.mb.resize((size_t)h->set.nmb);
    if (h->batch.packed()) d.ix.resize((size_t)h->set.nmb);
    if (!d.lv) d.lv.reset(new (std::nothrow) int16_t[(size_t)h->set.nmb * X264GPU_MB_LEVELS]);
    if (!d.lv) { xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: out of memory (download buffers)\n"); h->failed = true; return -1; }
    d.i_type = x264_type_of(pl.type); d.b_keyframe = idr; d.pts = pl.e.pts; d.img = pl.e.img;
    d.qp = f.pic.qp; d.qpm = f.pic.qpm; d.scenecut = pl.e.scenecut; memcpy(d.costs, pl.e.costs, sizeof(d.costs));
    d.q_type = quality_type(pl.type); d.q_poc = f.pic.poc;
    if (h->rc.reads_sizes()) { xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: a batched session cannot run rate control that reads the coded sizes\n"); h->failed = true; return -1; }
    d.dts = coded_dts(h, h->coded_count);
    Batch *b = &h->batch;
    const SliceParams sp = f.sp;
    const int slices = h->set.slices, threads = h->set.cavlc_threads, dev = h->device;
    const bool annexb = p.b_annexb != 0;
    const long my_launched = b->launched();
    d.hurry = false;
    d.th = std::thread([&d, b, bbuf, sp, slices, threads, annexb, idr, dev, my_launched]() {
        x264gpu_set_device(dev);
        x264gpu_level_index *ix = d.ix.empty() ? nullptr : d.ix.data();
        if (b->download(bbuf, d.mb.data(), d.lv.get(), d.err, ix, &d.q)) return;
        // the slices are written once the group's next round is on the device (the callers need the cores to get it there), or when the picture is asked for
        b->wait_launched(my_launched, d.hurry);
        b->timed(Batch::SLICES, my_launched, [&] { write_slices(d.out, d.off, d.types, sp, slices, d.mb.data(), d.lv.get(), annexb, idr, &d.stats, threads, ix); });
    });
    d.valid = true;
    h->dpb.commit();
    bmode_count(h, idr);
    h->defer_cur ^= 1;
    return publish_deferred(h, h->defer[h->defer_cur], pp_nal, pi_nal, pic_out);
}

// codes the next picture in coding order; returns the bytes of its NAL units, 0 when the queue still waits for input
static int encode_bmode(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out, bool flushing)
{
    const x264_param_t &p = h->param;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tb0 = now(), tb1 = 0;
    auto BPHASE = [&](int i) { tb1 = now(); h->t_b[i] += tb1 - tb0; tb0 = tb1; };
    const bool decided = h->slicetype.decide(flushing, h->rc);
    h->failed |= h->slicetype.failed;
    BPHASE(0);
    if (!decided) return flushing ? publish_deferred(h, h->defer[h->defer_cur ^ 1].valid ? h->defer[h->defer_cur ^ 1] : h->defer[h->defer_cur], pp_nal, pi_nal, pic_out) : 0;
    x264_t::PicPlan f;
    bmode_plan(h, f, h->gpu, h->coded_count, true);
    if (h->failed) return -1;          // (the macroblock-tree statistics file: a record of another picture type, said in the log)
    std::vector<int> vbv_types; bool vbv_sets = false, vbv_written = false;          // VBV: the access unit is written (and the picture coded again) before it is finished
    // launch: the group's round (its results downloaded here unless a helper thread does it: deferred), or this session's encoder and two downloads on the default stream
    const uint8_t *d_src = h->q_raw[(size_t)f.pl.e.slot];
    int bbuf = 0;
    const bool deferred = h->batch.overlap();
    if (h->batch.joined()) {
        std::string berr;
        if (h->batch.submit(d_src, f.pic, { f.d_offsets, f.d_mvs[0], f.d_mvs[1] }, &bbuf, berr) ||
            (!deferred && h->batch.download(bbuf, h->h_mb.data(), h->h_lv.data(), berr, nullptr, &h->hq[0]))) {
            xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: GPU hot path failed: %s\n", berr.c_str());
            h->failed = true;
            return -1;
        }
    } else
    for (;;) {
        if (x264gpu_encode_pictures(h->gpu, d_src, &f.pic, h->d_mb, h->d_lv, nullptr) != X264GPU_OK || (h->ql.flags && h->ql.queue(h->gpu, h->d_q, nullptr) != X264GPU_OK) ||
            (getenv("X264GPU_HOST_TIMING") && (x264gpu_stream_sync(nullptr), BPHASE(1), false)) || (h->ql.flags && x264gpu_memcpy_d2h(&h->hq[0], h->d_q, sizeof(h->hq[0]), nullptr) != X264GPU_OK) ||
            x264gpu_memcpy_d2h(h->h_mb.data(), h->d_mb, h->h_mb.size() * sizeof(x264gpu_mb), nullptr) != X264GPU_OK ||
            x264gpu_memcpy_d2h(h->h_lv.data(), h->d_lv, h->h_lv.size() * sizeof(int16_t), nullptr) != X264GPU_OK) {
            xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: GPU hot path failed: %s\n", x264gpu_last_error());
            h->failed = true;
            return -1;
        }
        if (!h->set.vbv) break;
        // the VBV's re-encode guard: the picture's exact size is known once its slices are written; one that would under-run the buffer (x264_ratecontrol_end's
        // "VBV underflow") is issued again — same x264gpu_pic, destination slot and source, which the device contract allows before any later picture — at a
        // quantiser raised by what its size asks for: bits fall roughly as 1 / qscale, and qscale doubles every 6.  The rate control's running state stays as
        // start() left it; everything that describes the picture afterwards describes the attempt that is emitted
        BPHASE(2);
        vbv_sets = bmode_write_au(h, f, vbv_types, h->h_mb.data(), h->h_lv.data());
        vbv_written = true;
        BPHASE(3);
        const double slice_bits = (double)h->out.size() * 8 - (double)h->last_vbv.overhead_bits, room = h->rc.buffer_fill;
        const int qp_max = h->rc.qp_ceiling();
        if (slice_bits <= room || f.pic.qp >= qp_max) break;
        const int step = room > 0 ? (int)ceil(6.0 * log2(slice_bits / (0.9 * room))) : qp_max;
        const int qp_new = clampi(f.pic.qp + (step > 1 ? step : 1), 1, qp_max);
        xlog(&p, X264_LOG_DEBUG, "VBV: frame %d took %.0f bits at qp %d with %.0f bits in the buffer: coded again at qp %d\n", f.pl.e.frame, slice_bits, f.pic.qp, room, qp_new);
        f.pic.qp = qp_new; f.pic.qpm = (float)qp_new; f.qpf = qp_new; f.sp.qp = qp_new;
        if (f.nal_ref_idc) h->rc.kept(f.pic.dst, f.qpf, f.pl.type);
        h->last_vbv.attempts++;
    }
    // a first pass that writes the macroblock-tree statistics file: the record of a kept picture, packed behind the picture on its stream (tree sessions name
    // q_tree for every kept picture; 2 bytes a macroblock come down)
    if (h->tstats.writing && f.nal_ref_idc && f.pl.type != PIC_B && !h->tstats.write_record(p, f.pl.type, f.d_offsets, nullptr)) { h->failed = true; return -1; }
    // --nr: the picture is accepted (the VBV guard is through with it) — its statistics join the session's state, the next picture's offsets follow
    if (h->nr.accepted(nullptr) != X264GPU_OK) { xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: nr update failed: %s\n", x264gpu_last_error()); h->failed = true; return -1; }
    BPHASE(2);
    if (const char *dd = getenv("X264GPU_DUMP_RECORDS")) {          // debugging aid: the records and levels of every coded picture, and what was asked of the device
        char fn[512];
        snprintf(fn, sizeof(fn), "%s/pic%04ld.bin", dd, h->coded_count);
        if (FILE *fp = fopen(fn, "wb")) {
            fwrite(&f.pic, sizeof(f.pic), 1, fp);
            fwrite(h->h_mb.data(), sizeof(x264gpu_mb), h->h_mb.size(), fp);
            fwrite(h->h_lv.data(), sizeof(int16_t), h->h_lv.size(), fp);
            std::vector<float> off((size_t)h->set.nmb, 0.f);          // ... and the per-macroblock quantiser offsets it was coded with (zeros: none handed in)
            if (f.d_offsets) x264gpu_memcpy_d2h(off.data(), f.d_offsets, off.size() * sizeof(float), nullptr);
            fwrite(off.data(), sizeof(float), off.size(), fp);
            fclose(fp);
        }
    }
    if (f.direct_auto_write) {
        // x264_encoder_frame_end ("somewhat arbitrary time constants"): the running counts decay once they exceed a picture's worth, then take this picture's
        int sc[2] = { 0, 0 };
        if (x264gpu_encoder_direct_scores(h->gpu, sc) != X264GPU_OK) { xlog(&p, X264_LOG_ERROR, "direct auto: %s\n", x264gpu_last_error()); h->failed = true; return -1; }
        if (h->direct_score[0] + h->direct_score[1] > h->set.mbw * h->set.mbh) for (int i = 0; i < 2; i++) h->direct_score[i] = h->direct_score[i] * 9 / 10;
        for (int i = 0; i < 2; i++) h->direct_score[i] += sc[i];
    }
    int size;
    if (deferred) size = bmode_defer(h, f, bbuf, pp_nal, pi_nal, pic_out);
    else {
        size = vbv_written ? bmode_finish_written(h, f, vbv_types, vbv_sets, h->h_mb.data(), pp_nal, pi_nal, pic_out) : bmode_finish(h, f, h->h_mb.data(), h->h_lv.data(), pp_nal, pi_nal, pic_out);
        h->dpb.commit();
    }
    BPHASE(3);
    return size;
}

// ---- several pictures of the session in flight ----
// issues the next picture of the coding order through a free launch context; false: nothing could be issued (no picture decided, no free context, no free slot)
static bool inflight_issue(x264_t *h, bool flushing)
{
    int ci = -1;
    for (int i = 0; i < (int)h->lctx.size(); i++) if (!h->lctx[(size_t)i].busy) { ci = i; break; }
    if (ci < 0) return false;
    if (!h->slicetype.decide(flushing, h->rc)) { h->failed |= h->slicetype.failed; return false; }
    // the slots the pictures in flight write or read stay out of the choice of a destination
    unsigned avoid = 0;
    for (const x264_t::PicPlan &q : h->fl) avoid |= q.slots_used;
    h->dpb.avoid = avoid;
    if (!h->dpb.has_free_slot()) return false;
    x264_t::LaunchCtx &c = h->lctx[(size_t)ci];
    x264_t::PicPlan f;
    f.ctx = ci;
    bmode_plan(h, f, c.gpu, h->coded_count + (long)h->fl.size(), false);
    const x264gpu_pic &pic = f.pic;
    // launch: on the context's stream, behind the pictures in flight that write a slot this picture reads (its references; their side data lives with the slot)
    f.slots_used = 1u << pic.dst;
    bool ok = true;
    for (int l = 0; l < 2 && ok; l++)
        for (int r = 0; r < pic.nref[l] && ok; r++) {
            const int sl = pic.slot[l][r];
            f.slots_used |= 1u << sl;
            const int w = h->slot_writer[sl];
            if (w >= 0 && w != ci) ok = x264gpu_stream_wait_event(c.stream, h->lctx[(size_t)w].ev) == X264GPU_OK;
        }
    // ... and behind the default stream: this picture's upload, its quantiser offsets and the lookahead's vectors were produced there
    ok = ok && x264gpu_event_record(h->ev_la, h->batch.upload_stream()) == X264GPU_OK && x264gpu_stream_wait_event(c.stream, h->ev_la) == X264GPU_OK;
    if (ok && h->batch.upload_stream()) ok = x264gpu_event_record(h->ev_la, nullptr) == X264GPU_OK && x264gpu_stream_wait_event(c.stream, h->ev_la) == X264GPU_OK;
    ok = ok && x264gpu_encode_pictures(c.gpu, h->q_raw[(size_t)f.pl.e.slot], &pic, c.d_mb, c.d_lv, c.stream) == X264GPU_OK &&
         (!h->ql.flags || h->ql.queue(c.gpu, c.d_q, c.stream) == X264GPU_OK) && x264gpu_event_record(c.ev, c.stream) == X264GPU_OK;
    if (!ok) { xlog(&h->param, X264_LOG_ERROR, "x264_encoder_encode: GPU hot path failed: %s\n", x264gpu_last_error()); h->failed = true; return false; }
    c.busy = true;
    h->slot_writer[pic.dst] = ci;
    h->dpb.commit();
    h->fl.push_back(f);
    return true;
}

// hands back the oldest picture in flight: waits for its launch context, downloads its records, writes its NAL units
static int inflight_retire(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out)
{
    x264_t::PicPlan f = h->fl.front();
    h->fl.pop_front();
    x264_t::LaunchCtx &c = h->lctx[(size_t)f.ctx];
    if (x264gpu_event_sync(c.ev) != X264GPU_OK || (h->ql.flags && x264gpu_memcpy_d2h(&h->hq[0], c.d_q, sizeof(h->hq[0]), c.stream) != X264GPU_OK) ||
        x264gpu_memcpy_d2h(h->h_mb.data(), c.d_mb, h->h_mb.size() * sizeof(x264gpu_mb), c.stream) != X264GPU_OK ||
        x264gpu_memcpy_d2h(h->h_lv.data(), c.d_lv, h->h_lv.size() * sizeof(int16_t), c.stream) != X264GPU_OK) {
        xlog(&h->param, X264_LOG_ERROR, "x264_encoder_encode: GPU hot path failed: %s\n", x264gpu_last_error());
        h->failed = true;
        return -1;
    }
    c.busy = false;
    if (h->slot_writer[f.pic.dst] == f.ctx) h->slot_writer[f.pic.dst] = -1;
    h->last_retired_slot = f.pic.dst;
    return bmode_finish(h, f, h->h_mb.data(), h->h_lv.data(), pp_nal, pi_nal, pic_out);
}

// ---- GOP slots with quantisers planned ahead (X264GPU_GOP_SLOTS_RC=1): the plan pass.  Every picture the slice-type decision releases is planned as encode_bmode plans
//      it — in the stream's coding order, on the session's own DPB model and rate control, nothing issued to a device encoder — and handed to the slots with the rows its
//      own encoder would have been told; a flush plans everything left, then the slots code their partly gathered batch.  Then the next coded picture, if there is one
static int encode_slots_rc(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out, bool flushing)
{
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    GopSlots &gs = h->gops;
    while (!gs.was_flushed()) {
        const double tb0 = now();
        const bool decided = h->slicetype.decide(flushing, h->rc);
        h->failed |= h->slicetype.failed;
        h->t_b[0] += now() - tb0;
        if (h->failed) return -1;
        if (!decided) break;
        x264_t::PicPlan f;
        bmode_plan(h, f, nullptr, h->plan_count, false);
        h->dpb.commit();
        h->plan_count++;
        h->t_b[4] += 1;
        const SliceType::Pic &pl = f.pl;
        const double tb1 = now();
        const int rc = gs.put_planned({ pl.e.frame, pl.type, f.pic.qp, f.pic.qpm, f.pic.direct_temporal, h->q_raw[(size_t)pl.e.slot], f.d_offsets, { f.d_mvs[0], f.d_mvs[1] } });
        h->t_b[1] += now() - tb1;
        h->failed |= gs.failed;
        if (rc < 0) return -1;
    }
    if (flushing) {
        const int rc = gs.flush();
        h->failed |= gs.failed;
        if (rc < 0) return -1;
    }
    return gop_slots_pop(h, pp_nal, pi_nal, pic_out);
}

static int encode_bmode_inflight(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_out, bool flushing)
{
    // issue what can be issued (a new picture's arrival may decide a mini-GOP: its closing picture, its B reference, its b pictures, as far as contexts and slots go) ...
    while (inflight_issue(h, flushing)) ;
    if (h->failed) return -1;
    if (h->fl.empty()) return 0;
    // ... and hand back the oldest picture once `inflight` pictures are out (x264's frame threads: i_thread_frames - 1 more calls of delay), when a decided picture
    // waits for a context or a slot, or when the input has ended; else this call returns nothing (a delayed frame).  The pictures behind the oldest keep running:
    // in the steady state a call issues one picture and waits for one that was issued inflight - 1 calls ago.
    if (!(flushing || (int)h->fl.size() >= h->set.inflight || !h->slicetype.queue().empty())) return 0;
    return inflight_retire(h, pp_nal, pi_nal, pic_out);
}

int x264_encoder_encode(x264_t *h, x264_nal_t **pp_nal, int *pi_nal, x264_picture_t *pic_in, x264_picture_t *pic_out)
{
    if (!h || !pp_nal || !pi_nal) return -1;
    *pi_nal = 0; *pp_nal = nullptr;
    if (h->failed) return -1;
    if (!pic_in) {      // flush: GOP-parallel batches, or the pictures still waiting in the lookahead queue, one per call
        if (h->set.slots_rc) return encode_slots_rc(h, pp_nal, pi_nal, pic_out, true);
        if (h->set.G > 1) return encode_gop_slots(h, pp_nal, pi_nal, nullptr, pic_out, false);
        if (h->set.dpbmode) return h->set.inflight > 1 ? encode_bmode_inflight(h, pp_nal, pi_nal, pic_out, true) : encode_bmode(h, pp_nal, pi_nal, pic_out, true);
        return h->queue.empty() ? 0 : encode_queued(h, pp_nal, pi_nal, pic_out, true);
    }
    const x264_param_t &p = h->param;
    const int w = p.i_width, ht = p.i_height;
    if ((pic_in->img.i_csp & X264_CSP_MASK) != X264_CSP_I420 || pic_in->img.i_plane < 3) {
        xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: input picture must be I420\n");
        return -1;
    }
    // Zero-copy input (x264gpu_host_input_i420): the caller (the VfW shell after the device-side colourspace conversion)
    // already placed a tight I420 picture in the encoder's device staging buffer.
    const bool resident = pic_in->img.plane[0] == h->d_in;
    if (h->set.slots_rc && h->gops.was_flushed()) { xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: pictures after a flush are not supported in GOP-parallel mode\n"); return -1; }
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = now(), t1;
#define PHASE(i) do { t1 = now(); h->t_phase[i] += t1 - t0; t0 = t1; } while (0)
    // ---- frame copy-in: three strided planes -> one tightly packed I420 buffer -> HBM (replaces x264_frame_copy_picture) ----
    uint8_t *dst = h->h_in.data();
    for (int pl = 0; pl < 3 && !resident; pl++) {
        int pw = pl ? w / 2 : w, ph = pl ? ht / 2 : ht;
        const uint8_t *src = pic_in->img.plane[pl];
        for (int y = 0; y < ph; y++, dst += pw, src += pic_in->img.i_stride[pl]) memcpy(dst, src, pw);
    }
    if (h->set.G > 1 && !h->set.slots_rc) return encode_gop_slots(h, pp_nal, pi_nal, pic_in, pic_out, resident);
    PHASE(0);
    // ---- the picture enters the lookahead queue (x264_lookahead_put_frame): upload, frame cost against the previous source picture,
    //      AQ offsets, slice-type decision (keyint / forced type / scenecut) — all causal, so they are taken on arrival ----
    const int slot = (int)(h->la_count % h->set.Q);
    uint8_t *d_raw = h->q_raw[(size_t)slot];
    void *const up = h->batch.upload_stream();          // (a batch session's: its pictures go up while the group's round runs on the compute stream)
    if ((!resident && x264gpu_memcpy_h2d(d_raw, h->h_in.data(), h->h_in.size(), up) != X264GPU_OK) ||
        (resident && d_raw != h->d_in && (x264gpu_memcpy_d2d(d_raw, h->d_in, h->h_in.size(), up) != X264GPU_OK || (up && x264gpu_stream_sync(up) != X264GPU_OK)))) {
        xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: upload failed: %s\n", x264gpu_last_error());
        return -1;
    }
    x264_t::QEntry e = {};
    e.pts = pic_in->i_pts; e.slot = slot; e.img = pic_in->img;
    bool idr = h->la_count == 0 || h->la_gop >= h->set.keyint || pic_in->i_type == X264_TYPE_IDR || pic_in->i_type == X264_TYPE_KEYFRAME, intra_pic = false;
    if (h->la) {
        if (h->tstats.reading) {          // (no frame costs: this session's lookahead object runs the AQ kernel alone)
            if (h->set.aq_strength != 0.f && x264gpu_lookahead_aq_offsets_mode(h->la, d_raw, h->set.aq_mode >= 2 ? h->set.aq_mode : 1, h->set.aq_strength, h->q_aq[(size_t)slot], nullptr) != X264GPU_OK) {
                xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: lookahead failed: %s\n", x264gpu_last_error());
                return -1;
            }
        } else
        if (x264gpu_lookahead_frame_cost(h->la, d_raw, h->la_count == 0, h->d_la, h->set.mbtree ? h->q_info[(size_t)slot] : nullptr, nullptr) != X264GPU_OK ||
            ((h->set.mbtree || h->slicetype.aq_costs || h->set.aq_mode >= 2) && h->set.aq_strength != 0.f && x264gpu_lookahead_aq_offsets_mode(h->la, d_raw, h->set.aq_mode >= 2 ? h->set.aq_mode : 1, h->set.aq_strength, h->q_aq[(size_t)slot], nullptr) != X264GPU_OK) ||
            x264gpu_memcpy_d2h(e.costs, h->d_la, sizeof(e.costs), nullptr) != X264GPU_OK) {
            xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: lookahead failed: %s\n", x264gpu_last_error());
            return -1;
        }
        if (!idr && p.i_scenecut_threshold > 0 && h->la_count > 0 && !h->tstats.reading) {
            // scenecut_internal: the bias grows with the distance from the last keyframe.  A cut at or beyond min-keyint becomes
            // an IDR picture, one inside min-keyint an I picture that keeps the references (x264_slicetype_decide).
            const int gop = h->la_gop, kmin = h->set.keyint_min, kmax = h->set.keyint;
            const double tmax = p.i_scenecut_threshold / 100.0, tmin = kmin == kmax ? tmax : tmax * 0.25;
            double bias;
            if (gop <= kmin / 4) bias = tmin / 4;
            else if (gop <= kmin) bias = tmin * gop / kmin;
            else bias = tmin + (tmax - tmin) * (gop - kmin) / (kmax - kmin);
            e.scenecut = (double)e.costs[1] >= (1.0 - bias) * (double)e.costs[0];
            if (e.scenecut) { if (gop >= kmin) idr = true; else intra_pic = true; }
        }
    }
    e.type = idr ? 2 : intra_pic ? 1 : 0;
    h->la_gop = idr ? 1 : h->la_gop + 1;
    h->la_count++;
    if (h->set.dpbmode) {
        SliceType::Frame be = {};
        be.pts = e.pts; be.frame = (int)(h->la_count - 1); be.slot = slot; be.forced = e.type; be.scenecut = e.scenecut; be.img = e.img;
        memcpy(be.costs, e.costs, sizeof(e.costs));
        if (pic_in->i_type == X264_TYPE_I) be.forced = 1;
        if (!h->slicetype.put(be, d_raw, pic_in->i_type == X264_TYPE_IDR || pic_in->i_type == X264_TYPE_KEYFRAME ? 2 : pic_in->i_type == X264_TYPE_I ? 1 : 0)) {
            xlog(&p, X264_LOG_ERROR, "x264_encoder_encode: lookahead failed: %s\n", x264gpu_last_error());
            return -1;
        }
        h->all_pts.push_back(e.pts);
        PHASE(1);
        const int size = h->set.slots_rc ? encode_slots_rc(h, pp_nal, pi_nal, pic_out, false) : h->set.inflight > 1 ? encode_bmode_inflight(h, pp_nal, pi_nal, pic_out, false) : encode_bmode(h, pp_nal, pi_nal, pic_out, false);
        PHASE(4);
        h->t_phase[5] += 1;
        return size;
    }
    h->queue.push_back(e);
    PHASE(1);
    if ((int)h->queue.size() <= h->set.L) return 0;                        // still filling the lookahead: no picture yet (codec.c:1693, size 0)
    const int size = encode_queued(h, pp_nal, pi_nal, pic_out, false);
    PHASE(4);
    h->t_phase[5] += 1;
#undef PHASE
    return size;
}

int x264_encoder_delayed_frames(x264_t *h) { return !h || h->failed ? 0 : h->set.slots_rc ? h->slicetype.delayed() + h->gops.delayed() : h->set.G > 1 ? h->gops.delayed() : h->set.dpbmode ? h->slicetype.delayed() + (int)h->fl.size() + (h->defer[0].valid ? 1 : 0) + (h->defer[1].valid ? 1 : 0) : (int)h->queue.size(); }

void x264_encoder_close(x264_t *h)
{
    if (!h) return;
    h->gops.close();
    join_gpu(h);
    for (auto &d : h->defer) join_deferred(h, d);
    if (getenv("X264GPU_HOST_TIMING") && h->t_phase[5] > 0)
        fprintf(stderr, "x264gpu host timing, ms per call over %.0f calls: copy-in %.2f, upload+lookahead %.2f, GPU %.2f, download %.2f, entropy %.2f\n", h->t_phase[5],
                1e3 * h->t_phase[0] / h->t_phase[5], 1e3 * h->t_phase[1] / h->t_phase[5], 1e3 * h->t_phase[2] / h->t_phase[5], 1e3 * h->t_phase[3] / h->t_phase[5], 1e3 * h->t_phase[4] / h->t_phase[5]);
    if (getenv("X264GPU_HOST_TIMING") && h->t_b[4] > 0)
        fprintf(stderr, "x264gpu host timing (DPB model), ms per picture over %.0f pictures: slice-type analysis %.2f, GPU hot path %.2f, download %.2f, entropy coding %.2f\n", h->t_b[4],
                1e3 * h->t_b[0] / h->t_b[4], 1e3 * h->t_b[1] / h->t_b[4], 1e3 * h->t_b[2] / h->t_b[4], 1e3 * h->t_b[3] / h->t_b[4]);
    h->ql.log_summary(h->param);
    h->rc.close();
    h->tstats.close(h->param);
    for (size_t i = 0; i < h->lctx.size(); i++) {
        x264_t::LaunchCtx &c = h->lctx[i];
        if (c.stream) { x264gpu_stream_sync(c.stream); x264gpu_stream_destroy(c.stream); }
        if (c.ev) x264gpu_event_destroy(c.ev);
        if (i > 0) { if (c.gpu) x264gpu_encoder_destroy(c.gpu); if (c.d_mb) x264gpu_free(c.d_mb); if (c.d_lv) x264gpu_free(c.d_lv); if (c.d_q) x264gpu_free(c.d_q); }
    }
    h->lctx.clear();
    if (h->ev_la) x264gpu_event_destroy(h->ev_la);
    h->batch.leave();
    h->nr.close();
    if (h->gpu) x264gpu_encoder_destroy(h->gpu);
    if (h->d_in) x264gpu_free(h->d_in);
    if (h->d_mb) x264gpu_free(h->d_mb);
    if (h->d_lv) x264gpu_free(h->d_lv);
    if (h->d_q) x264gpu_free(h->d_q);
    for (void *blk : h->q_block) if (blk) x264gpu_free(blk);          // the queue's slots (source pictures, lookahead records, AQ and tree offsets) are cuts of these
    if (h->d_tree) x264gpu_free(h->d_tree);
    if (h->la) x264gpu_lookahead_destroy(h->la);
    h->slicetype.close();
    if (h->d_la) x264gpu_free(h->d_la);
    delete h;
}

// what the slice-writing hooks are told of a picture, as SliceParams; the hooks without a DPB model add slice_type / frame_num / idr / num_ref, the others Dpb::fill
static SliceParams slice_params_from_args(int mbw, int mbh, int qp, int pic_init_qp, int log2_max_frame_num, int idr_pic_id, int disable_deblock_idc, int num_ref_default,
                                          int transform8x8_mode, int cabac)
{
    SliceParams sp = {};
    sp.mbw = mbw; sp.mbh = mbh; sp.qp = qp; sp.pic_init_qp = pic_init_qp; sp.log2_max_frame_num = log2_max_frame_num; sp.idr_pic_id = idr_pic_id;
    sp.num_ref_default = num_ref_default; sp.disable_deblock_idc = disable_deblock_idc; sp.transform8x8_mode = transform8x8_mode; sp.cabac = cabac;
    return sp;
}
static void set_ip_slice(SliceParams &sp, int slice_type, int frame_num, int idr, int num_ref)
{
    sp.slice_type = slice_type; sp.frame_num = frame_num; sp.idr = idr; sp.nal_ref_idc = idr ? 3 : 2; sp.num_ref = num_ref;
}
// the bytes a hook wrote, into the caller's buffer: their count, -1 when they do not fit
static int copy_out(const std::vector<uint8_t> &v, uint8_t *out, int cap)
{
    if ((int)v.size() > cap) return -1;
    memcpy(out, v.data(), v.size());
    return (int)v.size();
}
/* info[0..4] = frame_num, nal_ref_idc, n_mmco, reorder commands of list 0, of list 1 */
static int plan_out(const DpbPlan &p, x264gpu_pic *pic_out, int *info)
{
    *pic_out = p.pic;
    if (info) { info[0] = p.frame_num; info[1] = p.nal_ref_idc; info[2] = p.n_mmco; info[3] = p.reorder[0].n; info[4] = p.reorder[1].n; }
    return 0;
}

/* test/diagnostic hooks (not part of the x264 API): entropy-code caller-supplied records, fetch the GPU recon */
int x264host_write_slice(int mbw, int mbh, int slice_type, int qp, int pic_init_qp, int frame_num, int log2_max_frame_num,
                         int idr, int idr_pic_id, int disable_deblock_idc, int num_ref, int num_ref_default, int transform8x8_mode,
                         const x264gpu_mb *mbs, const int16_t *levels, uint8_t *out, int cap, int *skipped)
{
    SliceParams sp = slice_params_from_args(mbw, mbh, qp, pic_init_qp, log2_max_frame_num, idr_pic_id, disable_deblock_idc, num_ref_default, transform8x8_mode, 0);
    set_ip_slice(sp, slice_type, frame_num, idr, num_ref);
    std::vector<uint8_t> v;
    SliceStats stt = { 0 };
    write_slice(v, sp, mbs, levels, true, true, &stt, cavlc_threads_default(1));
    if (skipped) *skipped = stt.skip;
    return copy_out(v, out, cap);
}

// a whole picture of `slices` slices through either writer (tests: multi-slice pictures)
int x264host_write_picture(int mbw, int mbh, int slice_type, int qp, int pic_init_qp, int frame_num, int log2_max_frame_num,
                           int idr, int idr_pic_id, int disable_deblock_idc, int num_ref, int num_ref_default, int transform8x8_mode, int cabac, int slices,
                           const x264gpu_mb *mbs, const int16_t *levels, uint8_t *out, int cap, int *skipped)
{
    SliceParams sp = slice_params_from_args(mbw, mbh, qp, pic_init_qp, log2_max_frame_num, idr_pic_id, disable_deblock_idc, num_ref_default, transform8x8_mode, cabac);
    set_ip_slice(sp, slice_type, frame_num, idr, num_ref);
    sp.slices_plain = slices < 0;                 // -N: N slices as x264's --slices N codes them (filtered across), N: as its slice threads do
    if (slices < 0) slices = -slices;
    std::vector<uint8_t> v;
    SliceStats stt = { 0 };
    write_picture(v, nullptr, sp, slices, mbs, levels, true, true, &stt, 4);
    if (skipped) *skipped = stt.skip;
    return copy_out(v, out, cap);
}

// the same through the CABAC writer (tests: records from the CPU checker -> bytes -> checker decoder)
int x264host_write_slice_cabac(int mbw, int mbh, int slice_type, int qp, int pic_init_qp, int frame_num, int log2_max_frame_num,
                               int idr, int idr_pic_id, int disable_deblock_idc, int num_ref, int num_ref_default, int transform8x8_mode,
                               const x264gpu_mb *mbs, const int16_t *levels, uint8_t *out, int cap, int *skipped)
{
    SliceParams sp = slice_params_from_args(mbw, mbh, qp, pic_init_qp, log2_max_frame_num, idr_pic_id, disable_deblock_idc, num_ref_default, transform8x8_mode, 1);
    set_ip_slice(sp, slice_type, frame_num, idr, num_ref);
    std::vector<uint8_t> v;
    SliceStats stt = { 0 };
    write_slice(v, sp, mbs, levels, true, true, &stt, 1);
    if (skipped) *skipped = stt.skip;
    return copy_out(v, out, cap);
}

int x264host_write_headers_cabac(int width, int height, int level_idc, int log2_max_frame_num, int pic_init_qp, int chroma_qp_offset,
                                 uint32_t num_units_in_tick, uint32_t time_scale, int num_ref, int transform8x8_mode, int cabac, uint8_t *out, int cap);
int x264host_write_headers(int width, int height, int level_idc, int log2_max_frame_num, int pic_init_qp, int chroma_qp_offset,
                           uint32_t num_units_in_tick, uint32_t time_scale, int num_ref, int transform8x8_mode, uint8_t *out, int cap)
{
    return x264host_write_headers_cabac(width, height, level_idc, log2_max_frame_num, pic_init_qp, chroma_qp_offset, num_units_in_tick, time_scale, num_ref, transform8x8_mode, 0, out, cap);
}
int x264host_write_headers_cabac(int width, int height, int level_idc, int log2_max_frame_num, int pic_init_qp, int chroma_qp_offset,
                                 uint32_t num_units_in_tick, uint32_t time_scale, int num_ref, int transform8x8_mode, int cabac, uint8_t *out, int cap)
{
    SpsParams s = {};
    s.profile_idc = transform8x8_mode ? 100 : cabac ? 77 : 66; s.level_idc = level_idc; s.mbw = (width + 15) / 16; s.mbh = (height + 15) / 16;
    s.crop_right = s.mbw * 16 - width; s.crop_bottom = s.mbh * 16 - height; s.num_ref_frames = num_ref; s.log2_max_frame_num = log2_max_frame_num;
    s.fullrange = 0; s.colorprim = 2; s.transfer = 2; s.colmatrix = 2; s.vidformat = 5;
    s.num_units_in_tick = num_units_in_tick; s.time_scale = time_scale; s.constraint_set0 = !transform8x8_mode && !cabac; s.constraint_set1 = !transform8x8_mode;
    std::vector<uint8_t> v;
    write_sps(v, s, true);
    PpsParams pp = { 0, 0, cabac, num_ref, pic_init_qp, chroma_qp_offset, transform8x8_mode };
    write_pps(v, pp, true);
    return copy_out(v, out, cap);
}

/* ---- tests: the DPB model (dpb.hpp) and a slice writer driven by it, for B-picture streams built from the CPU checker's records ---- */
void *x264host_dpb_new(int frame_reference, int bframes, int b_pyramid, int log2_max_frame_num, int weightp)
{
    Dpb *d = new Dpb();
    d->configure(frame_reference, bframes, b_pyramid, log2_max_frame_num, weightp);
    return d;
}
void x264host_dpb_free(void *h) { delete (Dpb *)h; }
int x264host_dpb_info(void *h, int *max_dpb, int *num_reorder) { Dpb *d = (Dpb *)h; *max_dpb = d->max_dpb; *num_reorder = d->num_reorder; return d->slots(); }
int x264host_dpb_plan(void *h, int type, int frame, int n_follow, const int *follow_coded, const int *follow_frame, x264gpu_pic *pic_out, int *info)
{
    const DpbPlan &p = ((Dpb *)h)->plan(type, frame, n_follow, follow_coded, follow_frame);
    return plan_out(p, pic_out, info);
}
/* ... with a luma weight for reference 0 (x264_weights_analyse's result): w = { scale, denom, offset } */
int x264host_dpb_plan_w(void *h, int type, int frame, int n_follow, const int *follow_coded, const int *follow_frame, const int *w, x264gpu_pic *pic_out, int *info)
{
    Dpb::LumaWeight lw;
    if (w) { lw.on = 1; lw.scale = w[0]; lw.denom = w[1]; lw.offset = w[2]; }
    const DpbPlan &p = ((Dpb *)h)->plan(type, frame, n_follow, follow_coded, follow_frame, w ? &lw : nullptr);
    return plan_out(p, pic_out, info);
}
/* ... and chroma weights beside it: w = { scale, denom, offset, chroma denom, Cb on, Cb scale, Cb offset, Cr on, Cr scale, Cr offset } */
int x264host_dpb_plan_wc(void *h, int type, int frame, int n_follow, const int *follow_coded, const int *follow_frame, const int *w, x264gpu_pic *pic_out, int *info)
{
    Dpb::LumaWeight lw;
    lw.on = 1; lw.scale = w[0]; lw.denom = w[1]; lw.offset = w[2]; lw.cdenom = w[3];
    for (int c = 0; c < 2; c++) { lw.con[c] = w[4 + 3 * c]; lw.cscale[c] = w[5 + 3 * c]; lw.coffset[c] = w[6 + 3 * c]; }
    const DpbPlan &p = ((Dpb *)h)->plan(type, frame, n_follow, follow_coded, follow_frame, &lw);
    return plan_out(p, pic_out, info);
}
void x264host_dpb_commit(void *h) { ((Dpb *)h)->commit(); }
void x264host_dpb_set_direct(void *h, int temporal, int auto_write) { ((Dpb *)h)->set_direct(temporal, auto_write); }
int x264host_write_slice_dpb(void *h, int mbw, int mbh, int qp, int pic_init_qp, int log2_max_frame_num, int log2_max_poc_lsb, int idr_pic_id,
                             int disable_deblock_idc, int num_ref_default, int transform8x8_mode, const x264gpu_mb *mbs, const int16_t *levels,
                             uint8_t *out, int cap, int *skipped)
{
    SliceParams sp = slice_params_from_args(mbw, mbh, qp, pic_init_qp, log2_max_frame_num, idr_pic_id, disable_deblock_idc, num_ref_default, transform8x8_mode, 1);
    sp.log2_max_poc_lsb = log2_max_poc_lsb;
    ((Dpb *)h)->fill(sp);
    std::vector<uint8_t> v;
    SliceStats stt = { 0 };
    write_slice(v, sp, mbs, levels, true, true, &stt, 1);
    if (skipped) *skipped = stt.skip;
    return copy_out(v, out, cap);
}
// the same picture in `slices` slices (N: as x264's slice threads cut it, -N: as --slices N does)
int x264host_write_picture_dpb(void *h, int mbw, int mbh, int qp, int pic_init_qp, int log2_max_frame_num, int log2_max_poc_lsb, int idr_pic_id,
                               int disable_deblock_idc, int num_ref_default, int transform8x8_mode, int slices, const x264gpu_mb *mbs, const int16_t *levels,
                               uint8_t *out, int cap, int *skipped)
{
    SliceParams sp = slice_params_from_args(mbw, mbh, qp, pic_init_qp, log2_max_frame_num, idr_pic_id, disable_deblock_idc, num_ref_default, transform8x8_mode, 1);
    sp.log2_max_poc_lsb = log2_max_poc_lsb;
    sp.slices_plain = slices < 0;
    if (slices < 0) slices = -slices;
    ((Dpb *)h)->fill(sp);
    std::vector<uint8_t> v;
    SliceStats stt = { 0 };
    write_picture(v, nullptr, sp, slices > 1 ? slices : 1, mbs, levels, true, true, &stt, 1);
    if (skipped) *skipped = stt.skip;
    return copy_out(v, out, cap);
}
int x264host_write_headers_b(int width, int height, int level_idc, int log2_max_frame_num, int pic_init_qp, int chroma_qp_offset, uint32_t num_units_in_tick,
                             uint32_t time_scale, int num_ref_default, int transform8x8_mode, int cabac, int num_ref_frames, int log2_max_poc_lsb, int num_reorder,
                             int weighted_bipred_idc, int weighted_pred, uint8_t *out, int cap)
{
    SpsParams s = {};
    s.profile_idc = transform8x8_mode ? 100 : 77; s.level_idc = level_idc; s.mbw = (width + 15) / 16; s.mbh = (height + 15) / 16;
    s.crop_right = s.mbw * 16 - width; s.crop_bottom = s.mbh * 16 - height; s.num_ref_frames = num_ref_frames; s.log2_max_frame_num = log2_max_frame_num;
    s.fullrange = 0; s.colorprim = 2; s.transfer = 2; s.colmatrix = 2; s.vidformat = 5;
    s.num_units_in_tick = num_units_in_tick; s.time_scale = time_scale; s.constraint_set0 = 0; s.constraint_set1 = !transform8x8_mode;
    s.log2_max_poc_lsb = log2_max_poc_lsb; s.num_reorder_frames = num_reorder;
    std::vector<uint8_t> v;
    write_sps(v, s, true);
    PpsParams pp = { 0, 0, cabac, num_ref_default, pic_init_qp, chroma_qp_offset, transform8x8_mode };
    pp.weighted_bipred_idc = weighted_bipred_idc; pp.weighted_pred = weighted_pred;
    write_pps(v, pp, true);
    return copy_out(v, out, cap);
}

/* device pointer of the encoder's input staging buffer: a tight I420 picture (Y w*h, U, V).  A picture whose plane[0]
 * equals this pointer is encoded in place, without the host copy-in and upload (used by the VfW shell, vfw.cpp). */
uint8_t *x264gpu_host_input_i420(x264_t *h) { return h ? h->d_in : nullptr; }

long x264host_gop_slots_planned(x264_t *h) { return h && h->set.slots_rc ? h->gops.planned() : 0; }
int x264host_gop_slots_recon(x264_t *h, int slot, uint8_t *i420_out) { return h && h->set.G > 1 && i420_out ? h->gops.recon(slot, i420_out) : -1; }

int x264host_last_decision(x264_t *h, int *qp, int *scenecut, int32_t costs[4])
{
    if (!h) return -1;
    if (qp) *qp = h->last_qp;
    if (scenecut) *scenecut = h->last_scenecut;
    if (costs) memcpy(costs, h->last_costs, sizeof(h->last_costs));
    return 0;
}

/* tests: the second pass' plan — the quantiser scale init_pass2 gave every picture of the statistics file (display order), and what should have been spent before each;
 * returns the number of pictures planned (0: not a second pass) */
int x264host_last_vbv(x264_t *h, double out[12], int *planned_type, int *planned_satd, int cap)
{
    if (!h || !h->set.vbv || !h->last_vbv.valid) return -1;
    const x264_t::VbvInfo &v = h->last_vbv;
    if (out) {
        const double o[12] = { v.fill_before, v.fill_after, v.qp_novbv, v.qp_clipped, v.frame_size_planned, (double)v.attempts, (double)v.filler, v.qp_final,
                               (double)v.overhead_bits, h->rc.buffer_size, h->rc.vbv_max_rate, h->rc.frame_size_maximum };
        memcpy(out, o, sizeof(o));
    }
    int n = 0;
    while (n < RateControl::PLAN_MAX && v.planned.type[n] != RateControl::PLAN_END) n++;
    for (int i = 0; i <= n && i < cap; i++) {
        if (planned_type) planned_type[i] = i < n ? v.planned.type[i] : -1;
        if (planned_satd) planned_satd[i] = i < n ? v.planned.satd[i] : 0;
    }
    return n;
}
int x264host_pass2_plan(x264_t *h, double *new_qscale, double *expected_bits, int n)
{
    if (!h || !h->rc.pass2) return 0;
    for (int i = 0; i < n && i < h->rc.planned(); i++) { if (new_qscale) new_qscale[i] = h->rc.plan(i)->new_qscale; if (expected_bits) expected_bits[i] = h->rc.plan(i)->expected_bits; }
    return h->rc.planned();
}
/* tests: the float quantiser (x264 rc->qpm) the last coded picture's macroblock quantisers were rounded from; 0 = its integer quantiser */
float x264host_last_qpm(x264_t *h) { return h ? h->last_qpm : 0.f; }

int x264host_pictures_in_flight(x264_t *h) { return h ? h->set.inflight : 0; }

int x264host_last_quality(x264_t *h, double psnr[4], double *ssim, uint64_t ssd[3])
{
    if (!h || !h->ql.flags || !h->ql.have_last) return -1;
    if (psnr) memcpy(psnr, h->ql.last_psnr, sizeof(h->ql.last_psnr));
    if (ssim) *ssim = h->ql.last_ssim;
    if (ssd) memcpy(ssd, h->ql.last_ssd, sizeof(h->ql.last_ssd));
    return 0;
}

int x264host_nr_offsets(x264_t *h, uint16_t out[3][64])
{
    if (!h || !out) return -1;
    if (h->batch.joined()) return h->batch.nr_offsets(out);
    return h->nr.offsets(out);
}

int x264host_last_mb_qp_offsets(x264_t *h, float *dst, int n)
{
    if (!h || !dst || n != h->set.nmb) return -1;
    if (!h->last_offsets) return 0;
    if (x264gpu_stream_sync(nullptr) != X264GPU_OK || x264gpu_memcpy_d2h(dst, h->last_offsets, (size_t)n * sizeof(float), nullptr) != X264GPU_OK) return -1;
    return n;
}

int x264host_quality_summary(x264_t *h, char *buf, int cap)
{
    if (!h || !h->ql.flags || !buf || cap < 1) return -1;
    const std::string s = h->ql.summary(h->param);
    const size_t n = s.size() < (size_t)cap - 1 ? s.size() : (size_t)cap - 1;
    memcpy(buf, s.data(), n); buf[n] = 0;
    return (int)n;
}

int x264host_get_recon(x264_t *h, uint8_t *i420_out)
{
    if (!h || !h->gpu) return -1;
    join_gpu(h);                             // a pipelined session: this is the picture whose GPU stage ran last, not the one handed back last
    size_t n = (size_t)h->param.i_width * h->param.i_height * 3 / 2;
    uint8_t *d = nullptr;
    if (x264gpu_malloc((void **)&d, n) != X264GPU_OK) return -1;
    // (several pictures in flight: the picture handed back last — its slot is not reused before the next call issues a picture)
    int rc = h->set.inflight > 1 && h->last_retired_slot >= 0 ? x264gpu_encoder_get_recon_slot(h->gpu, 0, h->last_retired_slot, d, nullptr) : x264gpu_encoder_get_recon(h->gpu, 0, d, nullptr);
    if (rc == X264GPU_OK) rc = x264gpu_memcpy_d2h(i420_out, d, n, nullptr);
    x264gpu_free(d);
    return rc;
}

}  /* extern "C" */

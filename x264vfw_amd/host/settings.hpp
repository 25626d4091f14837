// settings.hpp — what a session really runs: x264_encoder_open's rules that turn the caller's x264_param_t into the effective parameters ([x264-upstream]
// encoder/encoder.c validate_parameters restated for this path) and into the constants the session is built from — toolset and slices, VBV and HRD, picture
// structure, the session's mode (DPB model, batch seat, GOP slots, pictures in flight), rate control, quantisers, profile and level, the lookahead window.
// One object per session behind one call: settle() runs once in x264_encoder_open, after the parameters are copied and before anything is created; it edits the
// session's copy of the parameters in place (x264_encoder_parameters reports them), sets the flags of the units it decides for and says every change in the
// log.  Nothing writes to the object afterwards: the session reads it through a const reference.  Plain C++ over x264_param_t and numbers: it sees neither
// x264_t nor the device (MbTreeStats::check_read reads the first pass' files), and the environment only through Env, read once at the top of settle().
#pragma once
#include "host.hpp"
#include "dpb.hpp"
#include "mbtreestats.hpp"
#include "ratecontrol.hpp"

namespace x264host {

struct Settings {
    // the environment's say in the rules (a variable that is not set: set false / 0)
    struct Env {
        bool batch_set = false; int batch = 0;          // X264GPU_BATCH=N
        int gop_slots = 0;                              // X264GPU_GOP_SLOTS=G: slice threads AND G GOP slots
        bool gop_slots_rc = false;                      // X264GPU_GOP_SLOTS_RC=1: CRF sessions with B pictures under --threads G
        bool inflight_set = false; int inflight = 0;    // X264GPU_INFLIGHT=N: pictures of one session in flight (default 4)
        bool dump_records = false;                      // X264GPU_DUMP_RECORDS: the debugging dump follows the serial path
        bool pipeline_off = false;                      // X264GPU_HOST_PIPELINE=0
        bool cavlc_threads_set = false; int cavlc_threads = 0;      // X264GPU_CAVLC_THREADS=N
        bool mbtree_stats = false;                      // X264GPU_MBTREE_STATS=1 (MbTreeStats::opted_in)
        bool qp_rd = false;                             // X264GPU_QP_RD=1: --subme 10 runs QP-RD where the session can (else it is subme 9, as without the variable)
        bool nr_any = false;                            // X264GPU_NR_ANY=1: --nr in every inter toolset the device has denoising kernels for (else today's rules)
    } env;

    int mbw = 0, mbh = 0, nmb = 0;
    int slices = 1;               // x264 slice threads: slices per picture (own wavefront + own NAL each)
    int slices_plain = 0;         // ... or x264 --slices N: the same split, filtered across the boundaries, up to one slice per macroblock row
    bool vbv = false;             // --vbv-maxrate / --vbv-bufsize run (single-pass CRF / ABR, one picture at a time on the DPB model)
    HrdParams hrd;                // --nal-hrd: the HRD in the VUI, buffering-period and picture-timing SEI messages (Annex C / D / E)
    int bframes = 0, bpyramid = 0;
    // dpbmode: the session runs on the DPB model (host/dpb.hpp) and x264gpu_encode_pictures — every session with B pictures, with VBV or in a batch, and sessions
    // without B pictures that use --weightp 2 (whose duplicate references need explicit lists); weightp: the effective --weightp
    bool dpbmode = false; int weightp = 0;
    int direct_mode = 1;          // --direct: 1 spatial, 2 temporal, 3 auto
    int keyint = 250, keyint_min = 25;
    int qp_i = 23, qp_p = 23, pic_init_qp = 26;
    int profile_idc = 66, level_idc = 40, log2_max_frame_num = 8, log2_max_poc_lsb = 0;
    bool qp_rd = false;           // x264's QP-RD runs (--subme 10 under X264GPU_QP_RD=1; settled in quantisers(), once AQ is); qprd_asked: --subme 10 / 11 came in and waits for that
    bool qprd_asked = false;
    bool nr_any = false;          // --nr was admitted on the extended toolset (X264GPU_NR_ANY=1 and a device library with x264gpu_encoder_set_nr_any): the session runs on the DPB model
    int cqo_without_psy_trellis = 0;      // the chroma quantiser offset without psy-trellis' share (what remains when psy-trellis gives way to nr)
    int G = 1;                    // --threads G: GOP slots (1: none)
    bool slots_rc = false;        // ... whose pictures the session plans ahead as a --threads 1 session does (X264GPU_GOP_SLOTS_RC=1)
    int inflight = 1;             // pictures of the session in flight (launch contexts)
    int dpb_slots = 0;            // DPB-model sessions: the device's picture slots (the DPB and one for every further picture in flight)
    int aq_mode = 0;              // --aq-mode (1 variance, 2 auto-variance, 3 auto-variance biased)
    float aq_strength = 0.f, tree_strength = 0.f;      // x264_adaptive_quant_frame's strength (mode 1: aq-strength * 1.0397f; 2 / 3: aq-strength), macroblock_tree_finish's 5.0f * (1.0f - qcomp)
    bool lookahead = false;       // the session has a lookahead object (costs for scenecut, CRF / ABR, --aq-mode 2 / 3, a second pass over the tree file)
    bool mbtree = false;          // macroblock-tree runs (it needs that object)
    int lookahead_asked = 0;      // rc-lookahead before the window below was fitted: what a batch group's key and the GOP slots' plan go by
    int L = 0, Q = 1;             // pictures held back; ring slots
    int st_wait = 0;              // x264 i_slicetype_length: the pictures the slice-type analysis waits for
    bool pipeline = false;        // threads-1 I / P sessions under CRF with pictures held back: the GPU stage of picture n + 1 overlaps the entropy coding of picture n
    int cavlc_threads = 1;        // row bands of a slice coded in parallel (threads 1 sessions; GOP-parallel ones use a thread per GOP)

    // batch_want: the group size the session asks for (Batch::want)
    void settle(x264_param_t &p, RateControl &rc, Dpb &dpb, MbTreeStats &tstats, int &batch_want);
    // what the device encoder(s) are created with: a copy of what settle() left here and in the parameters
    x264gpu_config device_config(const x264_param_t &p) const;
    // what settle() decided about the lookahead window and the VBV, said where the session's log has always said it: behind the device's own lines
    void log_lookahead(const x264_param_t &p) const;

private:
    int rc_lookahead_cut = 0, window_cut = 0;          // log_lookahead: rc-lookahead before it was cut to 60, the pictures the 128-picture window took (0: not cut)
    void toolset(x264_param_t &p);
    void vbv_rules(x264_param_t &p);
    void modes(x264_param_t &p, int &batch_want);
    void quantisers(x264_param_t &p, RateControl &rc, Dpb &dpb, MbTreeStats &tstats);
    void in_flight(x264_param_t &p, const RateControl &rc, Dpb &dpb, int batch_want);
    void lookahead_window(x264_param_t &p, RateControl &rc, const MbTreeStats &tstats);
};

}  // namespace x264host

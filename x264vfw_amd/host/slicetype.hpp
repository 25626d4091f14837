// slicetype.hpp — the picture types and the coding order of sessions on the DPB model ([x264-upstream] encoder/slicetype.c restated; checker twin: oracle/decide.py
// class Lookahead, tests/mbtree_walk.py).  One object per session behind three calls — open, put for every picture that arrives, decide before one is coded; plain
// C++ over x264_param_t, the rate control (read only) and the device's x264gpu_slicetype_* entries.
#pragma once
#include "dpb.hpp"          // (Dpb::LumaWeight, the weight a P picture is coded with)
#include "ratecontrol.hpp"
#include <deque>

namespace x264host {

struct SliceType {
    struct Frame { int64_t pts; int frame; int slot; int forced; int scenecut; int32_t costs[4]; x264_image_t img;      // forced: 0 auto, 1 I, 2 IDR
                   int type = 0; int b_scenecut = 1;         // the analysis: the type decided so far, "may still be a real scene cut"
                   Dpb::LumaWeight w;                        // x264_weights_analyse's luma weight of reference 0 when the picture is coded as P (--weightp)
                   RateControl::Planned planned;             // VBV with rc-lookahead: the types and costs of the pictures coded after this one (x264 i_planned_type / i_planned_satd)
                   float weighted_cost_delta[18] = { 0 }; }; // f_weighted_cost_delta[distance - 1]: weighted / unweighted cost where the fake analysis found a luma weight
    struct Pic { Frame e; int type; };                       // type: PIC_*

    // what the session settled before open(): ring slots, pictures held before a decision (x264 i_slicetype_length), toolset, views of its per-slot device arrays
    struct Setup { int slots, wait, mbw, mbh, bframes, bpyramid, weightp; bool mbtree, vbv; float aq_strength, tree_strength;
                   uint8_t *const *q_raw; float *const *q_aq, *const *q_tree; };
    // sessions that analyse (scenecut, --b-adapt 1 / 2, macroblock-tree, VBV lookahead) get x264's own lookahead structure on the device: frame costs of (p0, p1, b)
    // triples on the half-resolution planes, a queued picture's in the slot of the same number as its raw picture.  Sessions with a fixed picture structure run without
    // it: no fade weights, no lookahead vectors as search candidates (which also makes the sessions of a batch equal to the same sessions run alone).  false: said in the log
    bool open(x264_param_t &param, const RateControl &rc, const Setup &setup);
    void close();
    bool analyses() const { return st != nullptr; }
    bool aq_costs = false;               // AQ session without macroblock-tree: the rate control reads the AQ-weighted frame costs (i_cost_est_aq)
    bool failed = false;                 // a device call failed in decide(): the session is over
    // x264_lookahead_put_frame: the picture (ring slot fr.slot, d_raw on the device) joins the display-order queue; asked: the type the caller forced.  false: the device refused
    bool put(Frame &fr, const uint8_t *d_raw, int asked);
    // x264_slicetype_decide: closes the next mini-GOP when nothing waits to be coded -> whether the coding queue has a picture
    bool decide(bool flushing, const RateControl &rc);
    const std::deque<Pic> &queue() const { return coding; }          // coding order: the picture path takes the front and looks at the B pictures behind it
    Pic pop() { const Pic f = coding.front(); coding.pop_front(); return f; }
    int delayed() const { return (int)(bq.size() + coding.size()); }
    // fenc->lowres_mvs[list][distance - 1] of the picture in `slot` (device; nullptr: that search did not run)
    const int16_t *lowres_mvs(int slot, int list, int dist) const { return dist >= 1 && dist <= c.bframes + 1 ? x264gpu_slicetype_lowres_mvs(st, slot, list, dist) : nullptr; }

private:
    struct Window;                       // x264's frames[]: [0] the last non-B picture, [1 ..] the pictures waiting in display order; the analysis over them
    const x264_param_t *p = nullptr;
    x264gpu_slicetype *st = nullptr;
    Setup c = {};
    std::deque<Frame> bq;                // display order
    std::deque<Pic> coding;
    bool have_last_nonb = false; Frame last_nonb;
    int last_keyframe = 0;               // display index of the last IDR picture decided (x264 h->lookahead->i_last_keyframe)
    int badapt = 0;
    bool weightp_fake = false;           // x264 validate_parameters' X264_WEIGHTP_FAKE: --weightp 0 with macroblock-tree and psy: the lookahead still looks for fades, for the tree's sake alone

    void cost_failed();
    void reset_types();
    Dpb::LumaWeight weights_analyse(Frame &fenc, const Frame &ref, int dist, bool b_lookahead);
    int decide_types(const RateControl &rc);
    void close_minigop(int j, int closing);
};

}  // namespace x264host

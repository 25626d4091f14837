// batch.hpp — the cross-session batcher: a session's seat in a group of sessions that share one device encoder.
// The reference opens one CODEC / x264_t per stream (driverproc.c:110-128); the device is fast only when many streams are coded in lock-step
// (x264gpu_config.streams).  With X264GPU_BATCH=N in the environment, the first N sessions opened with the same geometry and toolset (and
// a fixed picture structure: no scenecut / b-adapt, so that picture k has the same type in all of them) form a group around one
// device encoder with N streams.  A session's x264_encoder_encode hands its picture to the group and waits; the call that completes the
// round launches the hot path for all streams; every caller then downloads its own records and entropy-codes its own stream on its own
// thread.  Each stream is coded exactly as a session of its own would code it (streams never interact): the bytes are the same.
// What a member's own lookahead decided for the picture travels with it — the per-macroblock quantiser offsets of macroblock-tree and --aq-mode 2 / 3, the
// low-resolution vectors the macroblock loop searches from: the group gathers its members' rows into the [streams][mb_count] arrays the device encoder
// takes (one x264gpu_gather_rows launch an array) in front of the round.  Sessions whose lookaheads differ in kind (tree or not, AQ mode, rc-lookahead,
// direct mode) never share a group.
// One object per session behind four calls — join at open, submit and download for every picture, leave at close — and the share of the session's helper
// thread (overlapping groups); plain C++ over the device's x264gpu_* entries.  The group, the registry of groups and their locks are batch.cpp's alone.
#pragma once
#include "host.hpp"
#include <atomic>
#include <functional>
#include <string>

namespace x264host {

struct BatchGroup;

struct Batch {
    int want = 0;                        // the group size the session asks for (X264GPU_BATCH=N of a session whose picture structure is fixed; 0: it runs on its own)

    // joins (or starts) the group of N sessions with this device configuration; false: setup failed (the device's last error set)
    // nr: the session's noise-reduction strength (0: none) — part of what a group's members have in common: every stream of the group's encoder then has its own
    // offsets, statistics and state, moved on behind every round; nr_any: the group's encoder denoises through x264gpu_encoder_set_nr_any (Settings::nr_any)
    // side: which of a picture's side inputs (SideInputs below) the session's lookahead can produce — offsets: quantiser offsets, mvs: low-resolution vectors — and
    // `key`, everything else that decides them (mbtree, aq-mode, rc-lookahead, the direct mode): members of a group agree in all three
    struct Side { bool offsets = false, mvs = false; int key = 0; };
    bool join(const x264gpu_config &cfg, int N, size_t insz, size_t nmb, int qflags, int nr, bool nr_any, const Side &side);
    // the registry lock, then the group's: the last member to go takes the group with it; a round the others were only waiting for this session to join is run first
    void leave();
    bool joined() const { return g != nullptr; }
    int index() const { return s; }      // the session's stream in the group's encoder
    int size() const;
    bool carries_offsets() const, carries_mvs() const;          // the group gathers its members' quantiser offsets / low-resolution vectors
    // overlap: the records / levels of round k are downloaded and entropy-coded (by a helper thread of every session) WHILE round k + 1 runs; every session hands its
    // pictures back one call later.  queued: the callers do not wait for the round either, it is queued on the group's own compute stream.  packed: the levels leave
    // the device packed (x264gpu_pack_levels): download() wants an index buffer and fills only the kept part of the levels
    bool overlap() const, queued() const, packed() const;
    // the session's upload stream (one of the group's, dealt round-robin): its pictures go up while the group's round runs on the compute stream.  nullptr outside a
    // group and in a group without upload streams (the uploads then wait on the default stream: slower, not wrong)
    void *upload_stream() const { return up; }

    // what a session on its own hands its device encoder for a picture (x264gpu_encoder_set_mb_qp_offsets / _set_lowres_mvs / _set_lowres_mvs1): device arrays of the
    // member's own, [mb_count] floats and [mb_count][2] int16, written on the default stream (the lookahead's) before submit; nullptr: none for this picture.
    // They must stay as they are until the round has run (the lookahead's ring keeps a slot for several pictures after it is coded)
    struct SideInputs { const float *d_offsets = nullptr; const int16_t *d_mvs0 = nullptr, *d_mvs1 = nullptr; };
    // hands picture `pic` (source d_src on the device) and its side inputs to the group and waits for the round that codes it; *buf = which pair of output buffers
    // holds the round's results
    int submit(const uint8_t *d_src, const x264gpu_pic &pic, const SideInputs &side, int *buf, std::string &err);
    // the session's records and levels of the round whose results lie in buffer pair `buf`
    // (h_ix: the group packs its levels — the member's index; h_lv then receives only the kept groups)
    int download(int buf, x264gpu_mb *h_mb, int16_t *h_lv, std::string &err, x264gpu_level_index *h_ix = nullptr, x264gpu_quality *h_q = nullptr);

    // --nr: the offsets the session's next picture will be denoised with (waits for the group's rounds on the device); -1 and zeros in a group without nr
    int nr_offsets(uint16_t out[3][64]);

    // ---- the helper thread of a session in an overlapping group: it downloads round k and writes its slices once round k + 1 is on the device, so that the host
    //      cores are the callers' while the next pictures are uploaded and submitted ----
    long launched();                     // the rounds whose kernels have been issued so far
    // sleeps until a round after `after` is on the device, `hurry` is set (wake() tells the sleepers to look) or the group has lost a member; 30 s at the most
    void wait_launched(long after, const std::atomic<bool> &hurry);
    void wake();                         // the group's sleepers look at their conditions again (nothing outside a group)
    // X264GPU_BATCH_TIMING=1: runs f and adds the time it took to the group's sums (SLICES also to those of round `round`, 1-based); outside a group f just runs
    enum Span { SLICES, JOIN };
    void timed(Span what, long round, const std::function<void()> &f);

private:
    BatchGroup *g = nullptr;
    int s = -1;
    void *up = nullptr;
};

}  // namespace x264host

// gopslots.hpp — the --threads G mode (G > 1; "GOP slots", "GOP-parallel mode"): G closed GOPs of the ONE stream are coded in lock-step on G stream slots of the
// device encoder(s).  A fixed keyint and a quantiser that does not read coded sizes (constant, zones, CRF decided on arrival) make the GOPs independent, so the
// bytes equal the serial session's (tests/test_shard_cpu.py, tests/test_gpu_host.py::test_gop_parallel_equals_serial).
// One object per session behind six calls — fit and open at open, put for every picture that arrives, flush when the input has ended, pop after either, close —
// plain C++ over x264_param_t, the device's x264gpu_* entries, Dpb and RateControl.  Writing an access unit (the sets, the SEI, the slices) is the picture path's,
// which every mode shares: the session hands a writer in at open.
//
// Frame -> (batch, slot, position).  Picture i of the stream belongs to GOP g = i / keyint at position t = i % keyint; GOP g runs on slot g % G of batch g / G.
// Pictures are uploaded into a position-major device ring, so the pictures of one position are contiguous = one device call.
// Slot -> device.  The G slots are dealt to the D visible devices (X264GPU_DEVICES caps D): slot s runs on device s % D as its local stream s / D.  Every device
// has its own encoder, ring and device-side record buffers; its slots' records land in the host download buffers from row `base` on (row_of / slot_of below).
// Closed GOPs are independent, so the devices exchange nothing.
// When a position is coded.  I / P sessions: position t, once the batch's last GOP has delivered it (every slot then has it), by one x264gpu_encode_frames per
// device.  Sessions with B pictures (--bframes N under a constant quantiser, --b-adapt 0, no scenecut): every slot is a closed GOP on the DPB model and runs the
// same plan — picture c of the coding order has the same type, lists and marking in every GOP — so coding position c is coded once the last GOP has delivered
// its picture (its references, in front of it in coding order, have then arrived too), by one x264gpu_encode_pictures per device that owns a slot.  At the
// flush the partly gathered batch is coded with the slots that have the position; with B pictures the stream's last, shorter GOP is coded alone, in a coding
// order and on a DPB model of its own.
// Output order.  I / P: stream order.  With B pictures: coding order inside every GOP, GOPs in stream order, with x264's pts / dts (the emitting code's).  One
// picture a call either way, through pop().
// Delay.  Nothing leaves before the first batch's last GOP starts delivering: (G - 1) * keyint calls, + bframes + 1 with B pictures (+ the lookahead's wait when the
// quantisers are planned ahead: put_planned).
//
// Threads.  put / flush / pop / close belong to one calling thread.  A position runs on that thread when there is one device, else on one host thread per device,
// joined before run_devices returns.  The access units of a position are then written by the CAVLC pool WHILE the next position runs on the devices.  A pool
// thread reads the session constants, the devices' `base` (row_of), the writer and the ONE download buffer pair its position landed in, and writes only the
// slotbuf entries of its own slots at its own position.  It never touches the bookkeeping: slot_have, the queues and the counters are written by the calling
// thread only, slot_have for a position when its pool has been joined.  Two download buffer pairs are used in turn: the pool of position n reads one while
// position n + 1 lands in the other; run_devices joins the pool of position n before position n + 2 may land in its pair.
#pragma once
#include "dpb.hpp"
#include "ratecontrol.hpp"
#include <deque>
#include <functional>
#include <thread>
#include <utility>

namespace x264host {

struct GopSlots {
    // a coded picture.  idr / i_type (X264_TYPE_*): the writer's.  ref_idc / disp: sessions with B pictures, where a slot index is a CODING position (nal_ref_idc of
    // its slices, its display index in its GOP).  index / pts: set by pop — the picture's place in the output order; I / P sessions: its pts
    struct Coded { std::vector<uint8_t> bytes; std::vector<size_t> off; std::vector<int> types; int idr = 0, ref_idc = -1, i_type = 0, disp = -1; long index = 0; int64_t pts = 0; };
    // the access unit of GOP `gop`'s picture of type PIC_* into cd, from the slot's records and levels; runs on pool threads, several at a time
    using Writer = std::function<void(Coded &cd, int pic_type, long gop, SliceParams sp, const x264gpu_mb *mb, const int16_t *lv)>;
    // what the session settled before open(): G (what fit returned), the structure, the toolset, the caller's device, the session-constant SliceParams, the writer
    struct Setup { int G, keyint, nmb, qp_i, qp_p, bframes, bpyramid, weightp, log2_max_frame_num, direct_mode; bool dpbmode; int device; SliceParams sp; Writer write;
                   bool planned = false, plan_offsets = false, plan_mvs = false; int plan_wait = 0; };      // planned: see Planned below; which rows its pictures can come with; the lookahead's wait (for the log)
    // a picture that arrives: tight I420 at `host`, or — resident — already in `staging`, the session's device buffer on the caller's device; the session's lookahead
    // and its four sums on that device (CRF)
    struct Input { const uint8_t *host; uint8_t *staging; bool resident; x264gpu_lookahead *la; int32_t *d_la; };

    // Quantisers planned ahead (X264GPU_GOP_SLOTS_RC=1: CRF sessions with B pictures).  The session runs its lookahead, its slice-type decision, a DPB model that follows
    // the serial stream and RateControl::start for every picture as a --threads 1 session would, in the stream's coding order, and hands each planned picture in here
    // instead of coding it: its source picture on the caller's device, what was decided for it, and the rows its own encoder would have been told (device arrays on the
    // caller's device; nullptr: none).  The lookahead recycles those arrays long before a slot codes the picture — up to (G - 1) x keyint pictures later — so the
    // picture goes into the ring and the rows into the plan store of the device that owns the slot (both device to device).  Slot G - 1's picture of a coding position
    // completes the position, which is then coded: every slot at its own quantisers, rows and direct mode.
    struct Planned { int frame, type, qp; float qpm; int direct_temporal; const uint8_t *d_src; const float *d_offsets; const int16_t *d_mvs[2]; };
    int put_planned(const Planned &pl);          // 0, or -1: said in the log
    long planned() const { return c.planned ? submitted : 0; }
    bool was_flushed() const { return flushed; }
    int recon(int slot, uint8_t *i420_out);          // tests: the reconstruction of the picture the slot's stream coded last, to the host; 0, or -1

    // the slot count the device ring (keyint x G pictures, plan_bytes of plan store beside each) allows: under 24 GB; p.i_threads follows, said in the log
    static int fit(x264_param_t &p, int keyint, size_t plan_bytes = 0);
    // the slots dealt to the devices — an encoder of cfg (its streams: the device's slots), record buffers and a ring per device — then the host side.  Leaves the
    // caller's device current.  false: said in the log (close() frees what exists)
    bool open(const x264_param_t &param, x264gpu_config cfg, RateControl &rc, const Setup &setup);
    // 0, or -1: said in the log.  After a device failure (failed) every later call returns -1 and nothing counts as delayed, so the caller's flush loop —
    // codec.c:1842-1856 — ends instead of spinning on pictures that will never be coded
    int put(const Input &in, int64_t pts);
    int flush();
    bool pop(Coded &c);                  // the next picture in output order, when it is coded
    int delayed() const { return (int)(submitted - emitted); }
    bool with_b() const { return gopb; }
    void close();                        // joins the pool, then frees what the devices hold
    bool failed = false;                 // a device call failed while a position was coded: the session is over

private:
    struct DevCtx {
        int dev = 0, nsl = 0, base = 0;  // device ordinal; slots it owns; its first row in the host download buffers
        x264gpu_encoder *gpu = nullptr;
        std::vector<x264gpu_encoder *> solo;      // quantisers planned ahead on a device library that takes lookahead vectors for one stream an encoder: an encoder a slot instead of gpu
        uint8_t *d_ring = nullptr;       // [keyint positions][nsl slots] tight I420 pictures of the batch being gathered
        x264gpu_mb *d_mb = nullptr; int16_t *d_lv = nullptr;
        // quantisers planned ahead: the plan store [keyint coding positions][nsl slots] of each array (offsets, vectors of list 0 / 1), the arrays gathered for the
        // position being coded [nsl], the device table of [3][nsl] row pointers the gather reads, the vectors' "absent" row (host/siderows.hpp)
        uint8_t *d_plan[3] = { nullptr, nullptr, nullptr }, *d_side[3] = { nullptr, nullptr, nullptr }; const void **d_tab = nullptr; int16_t *d_absent = nullptr;
    };
    // what the plan pass decided for a ring picture (slot * keyint + coding position); have: which rows lie in the plan store
    struct Rec { int type = -1, disp = 0, qp = 0; float qpm = 0.f; int direct_temporal = 0; bool have[3] = { false, false, false }; };
    std::vector<Rec> recs;
    struct GopDpb { Dpb dpb; int l0ref0poc[8] = { 0 }; };
    const x264_param_t *p = nullptr;
    RateControl *rc = nullptr;
    Setup c = {};
    size_t insz = 0;                     // bytes of a picture
    std::vector<DevCtx> devs;
    long submitted = 0, emitted = 0;     // pictures in / out
    int next_pos = 0;                    // first position of the current batch not yet coded
    bool flushed = false;                // the partly gathered batch has been coded (flush calls only drain after that)
    std::deque<Coded> ready;             // coded pictures [emitted, emitted + ready.size())
    std::deque<int64_t> pts;             // I / P sessions: pts of the pictures not yet emitted
    std::vector<Coded> slotbuf;          // G x keyint pictures of the batch being coded (index slot * keyint + position)
    std::vector<uint8_t> slot_have;      // which of them are coded AND joined
    std::vector<int8_t> gop_qp;          // CRF: the quantiser of every ring picture (slot * keyint + position), decided on arrival
    std::vector<float> gop_qpm;          // ... and its float quantiser (x264 rc->qpm)
    bool gopb = false;                   // B pictures: the slots run on the DPB model
    std::vector<std::pair<int, int>> gorder;      // coding order of a full GOP: (display index in the GOP, PIC_*)
    int gb_next = 0;                     // next coding position of the batch being gathered
    GopDpb gdpb;
    std::vector<std::thread> pool;       // CAVLC threads of the position coded last
    int pool_t = -1, pool_nslots = 0, pool_slot0 = 0;    // position / slot count / first slot they are coding
    std::vector<x264gpu_mb> h_mb[2];     // the two download buffer pairs, a row per slot
    std::vector<int16_t> h_lv[2];
    int dl = 0;                          // the pair the NEXT position lands in

    int D() const { return (int)devs.size(); }
    size_t row_of(int s) const { return (size_t)devs[(size_t)(s % D())].base + (size_t)(s / D()); }      // slot -> its row in the download buffers
    int slot_of(int local, int d) const { return local * D() + d; }                                      // device d's local stream -> slot
    void join_pool();
    int run_devices(int slot0, int nslots, bool owners_only, const std::function<bool(DevCtx &, int)> &launch, x264gpu_mb **hmb_out, int16_t **hlv_out);
    void start_pool(int pos, int slot0, int nslots, const std::function<void(int)> &work);
    int code_position(int batch, int t, int nslots_with_t);
    int code_position_b(int batch, int cpos, int slot0, int nslots, const std::vector<std::pair<int, int>> &order, GopDpb &gd);
    bool planned_side_rows(DevCtx &dc, int d, int cpos, int slot0, int nslots);
    void drain_coded();
};

}  // namespace x264host

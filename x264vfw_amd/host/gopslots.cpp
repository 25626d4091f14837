// gopslots.cpp — the --threads G mode (gopslots.hpp has the contract)
#include "gopslots.hpp"
#include "siderows.hpp"
#include <limits.h>
#include <stdlib.h>
#include <string>

namespace x264host {

// Coding order of a closed GOP of n pictures under --b-adapt 0 (x264_slicetype_decide with a fixed pattern, as bmode_decide walks it for a session
// without lookahead): an IDR picture, then runs of `bframes` B pictures closed by a P picture, the last picture always P; each closing picture first,
// then under --b-pyramid the middle B of a run of two or more as a reference, then the other B pictures in display order.
static std::vector<std::pair<int, int>> gop_coding_order(int n, int bframes, int bpyramid)
{
    std::vector<std::pair<int, int>> out;
    std::vector<int> run;
    for (int i = 0; i < n; i++) {
        const bool closes = i == 0 || (int)run.size() == bframes || i == n - 1;
        if (!closes) { run.push_back(i); continue; }
        out.push_back({ i, i == 0 ? PIC_IDR : PIC_P });
        const int j = (int)run.size(), bref = bpyramid && j > 1 ? (j - 1) / 2 : -1;
        if (bref >= 0) out.push_back({ run[(size_t)bref], PIC_BREF });
        for (int q = 0; q < j; q++) if (q != bref) out.push_back({ run[(size_t)q], PIC_B });
        run.clear();
    }
    return out;
}

int GopSlots::fit(x264_param_t &p, int keyint, size_t plan_bytes)
{
    int G = p.i_threads;
    const double pic = (double)p.i_width * p.i_height * 1.5 + (double)plan_bytes;
    while (G > 1 && pic * keyint * G > 24e9) G--;
    if (keyint >= (1 << 20)) G = 1;                  // "infinite" keyint: nothing to run in parallel
    if (G != p.i_threads) xlog(&p, X264_LOG_INFO, "threads %d -> %d (GOP ring of keyint %d pictures)\n", p.i_threads, G, keyint);
    p.i_threads = G;
    return G;
}

bool GopSlots::open(const x264_param_t &param, x264gpu_config cfg, RateControl &rc_, const Setup &setup)
{
    p = &param; rc = &rc_; c = setup;
    insz = (size_t)p->i_width * p->i_height * 3 / 2;
    const int G = c.G, K = c.keyint;
    int nd = x264gpu_device_count();
    if (const char *de = getenv("X264GPU_DEVICES")) { const int v = atoi(de); if (v >= 1 && v < nd) nd = v; }
    nd = clampi(nd, 1, G);
    devs.resize((size_t)nd);
    bool ok = true;
    int base = 0;
    for (int d = 0; d < nd && ok; d++) {
        DevCtx &dc = devs[(size_t)d];
        dc.dev = nd == 1 ? c.device : d; dc.nsl = (G - d + nd - 1) / nd; dc.base = base; base += dc.nsl;
        cfg.streams = dc.nsl;
        ok = x264gpu_set_device(dc.dev) == X264GPU_OK && x264gpu_encoder_create(&dc.gpu, &cfg) == X264GPU_OK &&
             x264gpu_malloc((void **)&dc.d_mb, (size_t)dc.nsl * c.nmb * sizeof(x264gpu_mb)) == X264GPU_OK &&
             x264gpu_malloc((void **)&dc.d_lv, (size_t)dc.nsl * c.nmb * X264GPU_MB_LEVELS * sizeof(int16_t)) == X264GPU_OK &&
             x264gpu_malloc((void **)&dc.d_ring, (size_t)dc.nsl * K * insz) == X264GPU_OK;
        if (ok && c.planned && (c.plan_offsets || c.plan_mvs)) {
            const size_t row = (size_t)c.nmb * 4;          // a float, or a vector of two int16, a macroblock
            for (int a = 0; a < 3 && ok; a++)
                if (a == 0 ? c.plan_offsets : c.plan_mvs)
                    ok = x264gpu_malloc((void **)&dc.d_plan[a], (size_t)dc.nsl * K * row) == X264GPU_OK && x264gpu_malloc((void **)&dc.d_side[a], (size_t)dc.nsl * row) == X264GPU_OK;
            ok = ok && x264gpu_malloc((void **)&dc.d_tab, 3 * (size_t)dc.nsl * sizeof(void *)) == X264GPU_OK && (!c.plan_mvs || (dc.d_absent = side_rows_absent((size_t)c.nmb)) != nullptr);
            // a device library may take the lookahead's vectors for encoders of one stream only (it says so when it is handed the array: nothing is read here).  The
            // device's slots then get an encoder each, coded one after the other: same pictures, same bytes, no lock-step on that device
            if (ok && c.plan_mvs && dc.nsl > 1) {
                if (x264gpu_encoder_set_lowres_mvs(dc.gpu, (const int16_t *)dc.d_side[1]) == X264GPU_OK) ok = x264gpu_encoder_set_lowres_mvs(dc.gpu, nullptr) == X264GPU_OK;
                else {
                    xlog(p, X264_LOG_INFO, "device %d: the device library takes lookahead vectors for one stream an encoder (%s): its %d GOP slots run on an encoder each\n", dc.dev, x264gpu_last_error(), dc.nsl);
                    x264gpu_encoder_destroy(dc.gpu); dc.gpu = nullptr;
                    cfg.streams = 1;
                    dc.solo.assign((size_t)dc.nsl, nullptr);
                    for (int l = 0; l < dc.nsl && ok; l++) ok = x264gpu_encoder_create(&dc.solo[(size_t)l], &cfg) == X264GPU_OK;
                }
            }
        }
    }
    const std::string err = ok ? "" : x264gpu_last_error();
    (void)x264gpu_set_device(c.device);
    if (!ok) { xlog(p, X264_LOG_ERROR, "GPU encoder setup failed: %s\n", err.c_str()); return false; }
    if (nd > 1) xlog(p, X264_LOG_INFO, "GOP slots on %d devices (%d + ... per device)\n", nd, devs[0].nsl);
    const size_t n = (size_t)G * K;
    gop_qp.assign(n, (int8_t)c.qp_p); gop_qpm.assign(n, 0.f);
    slotbuf.resize(n);
    slot_have.assign(n, 0);
    for (int i = 0; i < 2; i++) { h_mb[i].resize((size_t)G * c.nmb); h_lv[i].resize((size_t)G * c.nmb * X264GPU_MB_LEVELS); }
    if (c.dpbmode) {
        gopb = true;
        gorder = gop_coding_order(K, c.bframes, c.bpyramid);
        gdpb.dpb.configure(p->i_frame_reference, c.bframes, c.bpyramid, c.log2_max_frame_num, c.weightp);
        if (c.planned) {
            recs.assign(n, Rec());
            xlog(p, X264_LOG_INFO, "%d GOP slots in lock-step with B pictures (bframes %d, b-pyramid %d, quantisers planned ahead by the session's lookahead and rate control%s%s): pictures leave in coding order, %d calls late\n",
                 G, c.bframes, c.bpyramid, c.plan_offsets ? ", quantiser offsets" : "", c.plan_mvs ? ", lookahead vectors" : "", (G - 1) * K + c.plan_wait + 1);
        } else
        xlog(p, X264_LOG_INFO, "%d GOP slots in lock-step with B pictures (bframes %d, b-pyramid %d, constant quantiser): pictures leave in coding order, %d calls late\n", G, c.bframes, c.bpyramid, (G - 1) * K + c.bframes + 1);
    }
    return true;
}

void GopSlots::close()
{
    join_pool();          // (before anything it reads goes)
    for (auto &dc : devs) {
        if (devs.size() > 1) (void)x264gpu_set_device(dc.dev);
        if (dc.gpu) x264gpu_encoder_destroy(dc.gpu);
        for (x264gpu_encoder *e : dc.solo) if (e) x264gpu_encoder_destroy(e);
        if (dc.d_mb) x264gpu_free(dc.d_mb);
        if (dc.d_lv) x264gpu_free(dc.d_lv);
        if (dc.d_ring) x264gpu_free(dc.d_ring);
        for (int a = 0; a < 3; a++) { if (dc.d_plan[a]) x264gpu_free(dc.d_plan[a]); if (dc.d_side[a]) x264gpu_free(dc.d_side[a]); }
        if (dc.d_tab) x264gpu_free((void *)dc.d_tab);
        if (dc.d_absent) x264gpu_free(dc.d_absent);
    }
    if (devs.size() > 1) (void)x264gpu_set_device(c.device);
    devs.clear();          // (a second close finds nothing)
}

void GopSlots::join_pool()
{
    for (auto &th : pool) th.join();
    pool.clear();
    // only now do the pictures of that position count as coded
    for (int s = pool_slot0; s < pool_slot0 + pool_nslots; s++) slot_have[(size_t)s * c.keyint + pool_t] = 1;
    pool_nslots = 0; pool_slot0 = 0;
}

// One coding position of the slots [slot0, slot0 + nslots) on the devices: launch(dc, d) issues device d's encode call for its slots (false: it failed), the
// records and levels of those slots then land in the download buffer pair not in use (the error text is per thread: the first per device is kept).  The CAVLC
// pool of the position before is joined, it read the other pair.
// owners_only: devices that own none of the slots sit the position out (sessions with B pictures; the I / P mode launches every device).
// 0 and the buffers the position landed in, or -1 after a device failure (failed)
int GopSlots::run_devices(int slot0, int nslots, bool owners_only, const std::function<bool(DevCtx &, int)> &launch, x264gpu_mb **hmb_out, int16_t **hlv_out)
{
    x264gpu_mb *hmb = h_mb[dl].data();
    int16_t *hlv = h_lv[dl].data();
    dl ^= 1;
    const int nd = D();
    const size_t nmb = (size_t)c.nmb;
    std::vector<std::string> errs((size_t)nd);
    auto run_dev = [&](int d) {
        DevCtx &dc = devs[(size_t)d];
        bool mine = !owners_only;
        for (int s = slot0; s < slot0 + nslots; s++) mine |= s % nd == d;
        if (!mine) return;                                     // (the stream's last, shorter GOP is coded alone: only its device runs)
        const bool ok = (nd == 1 || x264gpu_set_device(dc.dev) == X264GPU_OK) && launch(dc, d) &&
                        x264gpu_memcpy_d2h(hmb + (size_t)dc.base * nmb, dc.d_mb, (size_t)dc.nsl * nmb * sizeof(x264gpu_mb), nullptr) == X264GPU_OK &&
                        x264gpu_memcpy_d2h(hlv + (size_t)dc.base * nmb * X264GPU_MB_LEVELS, dc.d_lv, (size_t)dc.nsl * nmb * X264GPU_MB_LEVELS * sizeof(int16_t), nullptr) == X264GPU_OK;
        if (!ok) errs[(size_t)d] = std::string("device ") + std::to_string(dc.dev) + ": " + x264gpu_last_error();
    };
    if (nd == 1) run_dev(0);
    else {
        std::vector<std::thread> ths;
        for (int d = 0; d < nd; d++) ths.emplace_back(run_dev, d);
        for (auto &th : ths) th.join();
    }
    join_pool();
    for (int d = 0; d < nd; d++)
        if (!errs[(size_t)d].empty()) {
            xlog(p, X264_LOG_ERROR, "x264_encoder_encode: GPU hot path failed: %s\n", errs[(size_t)d].c_str());
            failed = true;
            return -1;
        }
    *hmb_out = hmb; *hlv_out = hlv;
    return 0;
}

// starts the CAVLC pool over the slots [slot0, slot0 + nslots) of position `pos`: work(s) writes slot s' access unit
void GopSlots::start_pool(int pos, int slot0, int nslots, const std::function<void(int)> &work)
{
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthr = (int)(hw ? (hw < (unsigned)nslots ? hw : (unsigned)nslots) : 1);
    pool_t = pos; pool_nslots = nslots; pool_slot0 = slot0;
    for (int th = 0; th < nthr; th++)
        pool.emplace_back([work, th, nthr, slot0, nslots]() { for (int s = slot0 + th; s < slot0 + nslots; s += nthr) work(s); });
}

// Quantisers planned ahead, in front of device d's call for coding position cpos (on its thread, its device current): the rows of its slots' pictures out of the plan
// store become the encoder's [nsl][mb_count] arrays — offsets, vectors of list 0, vectors of list 1 — one gather an array on the stream the call runs on.  A slot
// coded along and thrown away takes the first asked slot's rows; a slot without vectors among slots with them the "absent" row.  false: the device's last error set
bool GopSlots::planned_side_rows(DevCtx &dc, int d, int cpos, int slot0, int nslots)
{
    const size_t N = (size_t)dc.nsl, row = (size_t)c.nmb * 4, K = (size_t)c.keyint;
    std::vector<const void *> tab(3 * N, nullptr);
    bool any[3] = { false, false, false };
    int mine0 = -1;          // the first asked slot this device owns (it owns one, or it would sit the position out): the plan store is per device
    for (int s = slot0; s < slot0 + nslots && mine0 < 0; s++) if (s % D() == d) mine0 = s;
    if (mine0 < 0) return true;
    for (size_t l = 0; l < N; l++) {
        int s = slot_of((int)l, d);
        if (s < slot0 || s >= slot0 + nslots) s = mine0;
        const Rec &r = recs[(size_t)s * K + (size_t)cpos];
        for (int a = 0; a < 3; a++)
            if (r.have[a]) { tab[(size_t)a * N + l] = dc.d_plan[a] + ((size_t)cpos * N + (size_t)(s / D())) * row; any[a] = true; }
    }
    for (int a = 1; a < 3; a++) if (any[a]) for (size_t l = 0; l < N; l++) if (!tab[(size_t)a * N + l]) tab[(size_t)a * N + l] = dc.d_absent;
    if ((any[0] || any[1] || any[2]) && !side_rows_gather(tab.data(), any, dc.d_tab, dc.d_side, N, row, nullptr, nullptr)) return false;
    return x264gpu_encoder_set_mb_qp_offsets(dc.gpu, any[0] ? (const float *)dc.d_side[0] : nullptr) == X264GPU_OK &&
           x264gpu_encoder_set_lowres_mvs(dc.gpu, any[1] ? (const int16_t *)dc.d_side[1] : nullptr) == X264GPU_OK &&
           x264gpu_encoder_set_lowres_mvs1(dc.gpu, any[2] ? (const int16_t *)dc.d_side[2] : nullptr) == X264GPU_OK;
}

// Sessions with B pictures: coding position cpos of `order` for the slots [slot0, slot0 + nslots) of batch `batch` — the plan from the DPB model (the same for
// every slot), one x264gpu_encode_pictures per device that owns one of the slots.  0, or -1 after a device failure
int GopSlots::code_position_b(int batch, int cpos, int slot0, int nslots, const std::vector<std::pair<int, int>> &order, GopDpb &gd)
{
    const int G = c.G, K = c.keyint, disp = order[(size_t)cpos].first, type = order[(size_t)cpos].second;
    // the disposable pictures coded right behind this one (x264_reference_hierarchy_reset looks at them)
    int fc[16], ff[16], nf = 0;
    for (size_t i = (size_t)cpos + 1; i < order.size() && nf < 16 && order[i].second == PIC_B; i++) { fc[nf] = (int)i; ff[nf] = order[i].first; nf++; }
    const DpbPlan plan = gd.dpb.plan(type, disp, nf, fc, ff, nullptr);
    x264gpu_pic pic = plan.pic;
    // quantisers planned ahead: what the plan pass decided for the slot's picture (a slot coded along and thrown away: the first asked slot's)
    auto rec_of = [&](int s) -> const Rec & { return recs[(size_t)(s >= slot0 && s < slot0 + nslots ? s : slot0) * K + (size_t)cpos]; };
    if (c.planned) {
        if (type == PIC_B || type == PIC_BREF) { pic.direct_temporal = rec_of(slot0).direct_temporal; pic.direct_auto = 0; gd.dpb.set_direct(pic.direct_temporal, 0); }
    } else
    if ((type == PIC_B || type == PIC_BREF) && c.direct_mode == 2) {
        // x264 slice_header_init: temporal direct prediction only when the co-located picture's reference 0 is this picture's reference 0
        const bool temporal = pic.nref[0] && pic.nref[1] && gd.l0ref0poc[pic.slot[1][0]] == plan.list_poc[0][0];
        pic.direct_temporal = temporal; pic.direct_auto = 0;
        gd.dpb.set_direct(pic.direct_temporal, 0);
    }
    if (plan.nal_ref_idc) gd.l0ref0poc[pic.dst] = pic.nref[0] ? plan.list_poc[0][0] : INT_MIN;
    // constant quantiser by picture type, a zone shifts it by the picture's display index in the stream (a slot coded along and thrown away: the type's)
    std::vector<int> qps((size_t)G, rc->qp_constant[type]);
    // (quantisers planned ahead: RateControl::start ran in the plan pass, in the stream's coding order; a slot's float quantiser and direct mode travel in its x264gpu_pic)
    std::vector<float> qpms((size_t)G, 0.f);
    std::vector<uint8_t> temporal((size_t)G, (uint8_t)pic.direct_temporal);
    for (int s = 0; s < G; s++) {
        if (c.planned) { const Rec &r = rec_of(s); qps[(size_t)s] = r.qp; qpms[(size_t)s] = r.qpm; if (type == PIC_B || type == PIC_BREF) temporal[(size_t)s] = (uint8_t)r.direct_temporal; }
        else if (s >= slot0 && s < slot0 + nslots) qps[(size_t)s] = rc->start(type, (int)(((long)batch * G + s) * K + disp));
    }
    SliceParams sp = c.sp;
    gd.dpb.fill(sp);
    gd.dpb.commit();
    x264gpu_mb *hmb; int16_t *hlv;
    auto launch = [&](DevCtx &dc, int d) {
        std::vector<x264gpu_pic> pics((size_t)dc.nsl, pic);
        for (int l = 0; l < dc.nsl; l++) {
            const size_t s = (size_t)slot_of(l, d);
            pics[(size_t)l].qp = qps[s];
            if (c.planned) { pics[(size_t)l].qpm = qpms[s]; pics[(size_t)l].direct_temporal = temporal[s]; }
        }
        if (!dc.solo.empty()) {
            // an encoder a slot (open() says when): the asked slots one after the other, each told its own rows where they lie in the plan store
            const size_t row = (size_t)c.nmb * 4;
            for (int l = 0; l < dc.nsl; l++) {
                const int s = slot_of(l, d);
                if (s < slot0 || s >= slot0 + nslots) continue;
                const Rec &r = recs[(size_t)s * K + (size_t)cpos];
                const uint8_t *rows[3];
                for (int a = 0; a < 3; a++) rows[a] = r.have[a] ? dc.d_plan[a] + ((size_t)cpos * dc.nsl + (size_t)l) * row : nullptr;
                x264gpu_encoder *e = dc.solo[(size_t)l];
                if (x264gpu_encoder_set_mb_qp_offsets(e, (const float *)rows[0]) != X264GPU_OK || x264gpu_encoder_set_lowres_mvs(e, (const int16_t *)rows[1]) != X264GPU_OK ||
                    x264gpu_encoder_set_lowres_mvs1(e, (const int16_t *)rows[2]) != X264GPU_OK ||
                    x264gpu_encode_pictures(e, dc.d_ring + ((size_t)disp * dc.nsl + (size_t)l) * insz, &pics[(size_t)l], dc.d_mb + (size_t)l * c.nmb,
                                            dc.d_lv + (size_t)l * c.nmb * X264GPU_MB_LEVELS, nullptr) != X264GPU_OK) return false;
            }
            return true;
        }
        if (c.planned && !planned_side_rows(dc, d, cpos, slot0, nslots)) return false;
        return x264gpu_encode_pictures(dc.gpu, dc.d_ring + (size_t)disp * dc.nsl * insz, pics.data(), dc.d_mb, dc.d_lv, nullptr) == X264GPU_OK;
    };
    if (run_devices(slot0, nslots, true, launch, &hmb, &hlv) < 0) return -1;
    const int ref_idc = plan.nal_ref_idc;
    start_pool(cpos, slot0, nslots, [this, batch, cpos, disp, type, hmb, hlv, qps, temporal, sp, ref_idc](int s) {
        const size_t row = row_of(s);
        Coded &cd = slotbuf[(size_t)s * c.keyint + cpos];
        cd.ref_idc = ref_idc; cd.disp = disp;
        SliceParams sps = sp;
        sps.qp = qps[(size_t)s];
        if (c.planned && (type == PIC_B || type == PIC_BREF)) sps.direct_spatial = !temporal[(size_t)s];
        c.write(cd, type, (long)batch * c.G + s, sps, hmb + row * c.nmb, hlv + row * c.nmb * X264GPU_MB_LEVELS);
    });
    return 0;
}

// I / P sessions: position t of the slots [0, nslots_with_t) of batch `batch`, one x264gpu_encode_frames per device.  0, or -1 after a device failure
int GopSlots::code_position(int batch, int t, int nslots_with_t)
{
    const int st = t == 0 ? X264GPU_SLICE_I : X264GPU_SLICE_P, G = c.G, K = c.keyint;
    std::vector<int8_t> qps; std::vector<float> qpms;
    if (rc->crf || (!rc->abr && !rc->zones.empty())) {
        // CRF: decided when the pictures arrived; constant quantiser with zones: slot s of this batch holds picture (batch * G + s) * keyint + t of the stream
        qps.assign((size_t)G, (int8_t)(t == 0 ? c.qp_i : c.qp_p)); qpms.assign((size_t)G, 0.f);
        for (int s = 0; s < nslots_with_t; s++)
            if (rc->crf) { qps[(size_t)s] = gop_qp[(size_t)s * K + t]; qpms[(size_t)s] = gop_qpm[(size_t)s * K + t]; }
            else qps[(size_t)s] = (int8_t)rc->start(t == 0 ? PIC_IDR : PIC_P, (int)(((long)batch * G + s) * K + t));
    }
    // every device codes position t of its slots: GPU + download run while the CAVLC threads of the previous position are still coding from the other buffer pair
    x264gpu_mb *hmb; int16_t *hlv;
    auto launch = [&](DevCtx &dc, int d) {
        if (!qps.empty()) {
            std::vector<int8_t> q((size_t)dc.nsl); std::vector<float> qm((size_t)dc.nsl);
            for (int l = 0; l < dc.nsl; l++) { q[(size_t)l] = qps[(size_t)slot_of(l, d)]; qm[(size_t)l] = qpms[(size_t)slot_of(l, d)]; }
            if (x264gpu_encoder_set_stream_qpms(dc.gpu, q.data(), qm.data()) != X264GPU_OK) return false;
        }
        return x264gpu_encode_frames(dc.gpu, dc.d_ring + (size_t)t * dc.nsl * insz, st, dc.d_mb, dc.d_lv, nullptr) == X264GPU_OK;
    };
    if (run_devices(0, nslots_with_t, false, launch, &hmb, &hlv) < 0) return -1;
    start_pool(t, 0, nslots_with_t, [this, batch, t, st, hmb, hlv, qps](int s) {
        const size_t row = row_of(s);
        const bool idr = t == 0;
        SliceParams sp = c.sp;
        sp.slice_type = st; sp.qp = !qps.empty() ? (int)qps[(size_t)s] : idr ? c.qp_i : c.qp_p;
        sp.frame_num = t & ((1 << c.log2_max_frame_num) - 1); sp.idr = idr; sp.nal_ref_idc = idr ? 3 : 2;
        sp.num_ref = t < p->i_frame_reference ? (t > 0 ? t : 1) : p->i_frame_reference;
        c.write(slotbuf[(size_t)s * c.keyint + t], idr ? PIC_IDR : PIC_P, (long)batch * c.G + s, sp, hmb + row * c.nmb, hlv + row * c.nmb * X264GPU_MB_LEVELS);
    });
    return 0;
}

// coded pictures move to the ordered output queue once every earlier picture is there.  slotbuf is indexed inside a batch
// (slot * keyint + position); an entry is reused by the next batch only long after it was drained.
void GopSlots::drain_coded()
{
    const long K = c.keyint, per_batch = (long)c.G * K;
    for (long g = emitted + (long)ready.size(); g < submitted; g++) {
        const long j = g % per_batch;
        const size_t idx = (size_t)(j / K) * K + (size_t)(j % K);
        if (!slot_have[idx]) break;                          // not coded yet (or its CAVLC threads have not been joined)
        ready.push_back(std::move(slotbuf[idx]));
        slot_have[idx] = 0;
    }
}

int GopSlots::put(const Input &in, int64_t pic_pts)
{
    const int G = c.G, K = c.keyint;
    const long per_batch = (long)G * K;
    if (failed) return -1;
    if (flushed) { xlog(p, X264_LOG_ERROR, "x264_encoder_encode: pictures after a flush are not supported in GOP-parallel mode\n"); return -1; }
    const long i = submitted, b = i / per_batch, r = i % per_batch;
    const int s = (int)(r / K), t = (int)(r % K);
    // (a new batch only starts gathering once the previous one is fully coded: its last position ran when its last picture arrived)
    DevCtx &dc = devs[(size_t)(s % D())];
    uint8_t *dst = dc.d_ring + ((size_t)t * dc.nsl + (size_t)(s / D())) * insz;
    const void *src = in.resident ? (const void *)in.staging : (const void *)in.host;
    if ((in.resident ? x264gpu_memcpy_d2d(dst, src, insz, nullptr) : x264gpu_memcpy_h2d(dst, src, insz, nullptr)) != X264GPU_OK) {
        xlog(p, X264_LOG_ERROR, "x264_encoder_encode: upload failed: %s\n", x264gpu_last_error());
        return -1;
    }
    // the lookahead lives on the caller's device: with several devices the picture also goes to the staging buffer there
    const uint8_t *la_src = dst;
    if (rc->crf && D() > 1 && dc.dev != c.device) {
        if (!in.resident && x264gpu_memcpy_h2d(in.staging, src, insz, nullptr) != X264GPU_OK) { xlog(p, X264_LOG_ERROR, "x264_encoder_encode: upload failed: %s\n", x264gpu_last_error()); return -1; }
        la_src = in.staging;
    }
    if (rc->crf) {
        // CRF: the picture's quantiser follows from the lookahead costs and the pictures before it, all known now (decided by its display index)
        int32_t costs[4];
        if (x264gpu_lookahead_frame_cost(in.la, la_src, i == 0, in.d_la, nullptr, nullptr) != X264GPU_OK ||
            x264gpu_memcpy_d2h(costs, in.d_la, sizeof(costs), nullptr) != X264GPU_OK) {
            xlog(p, X264_LOG_ERROR, "x264_encoder_encode: lookahead failed: %s\n", x264gpu_last_error());
            return -1;
        }
        double qpf;
        gop_qp[(size_t)s * K + t] = (int8_t)rc->start(t == 0 ? PIC_IDR : PIC_P, (int)i, costs, nullptr, &qpf);
        gop_qpm[(size_t)s * K + t] = near_qpm(qpf, gop_qp[(size_t)s * K + t]);
    }
    if (!gopb) pts.push_back(pic_pts);
    submitted++;
    if (s == G - 1 && gopb) {
        // every slot holds display picture t now: the coding positions whose picture (and, being in coding order behind their closing picture,
        // whose references) have arrived
        if (t == 0) gb_next = 0;
        while (gb_next < K && gorder[(size_t)gb_next].first <= t) {
            if (code_position_b((int)b, gb_next, 0, G, gorder, gdpb) < 0) return -1;
            gb_next++;
        }
        next_pos = t + 1 == K ? 0 : t + 1;
    } else if (s == G - 1) {                                   // the batch's last GOP delivers position t: every slot has it
        if (code_position((int)b, t, G) < 0) return -1;
        next_pos = t + 1 == K ? 0 : t + 1;
    } else if (!pool.empty()) join_pool();                     // gathering phase: the last position's CAVLC had a whole call to finish
    drain_coded();
    return 0;
}

// Quantisers planned ahead: the stream's next picture in CODING order (closed GOPs: GOP by GOP, so the slot and the coding position follow from the count).  Its
// source and rows move to the device that owns the slot; when slot G - 1 delivers the coding position the full GOP has there, the position is coded.  A picture of
// slot G - 1 that is not the full GOP's (the stream's last, shorter GOP, known at the flush only) ends the lock-step rounds: flush() codes that GOP alone
int GopSlots::put_planned(const Planned &pl)
{
    const int G = c.G, K = c.keyint;
    const long per_batch = (long)G * K;
    if (failed) return -1;
    if (flushed) { xlog(p, X264_LOG_ERROR, "x264_encoder_encode: pictures after a flush are not supported in GOP-parallel mode\n"); return -1; }
    const long i = submitted, b = i / per_batch, r = i % per_batch;
    const int s = (int)(r / K), cpos = (int)(r % K), t = pl.frame % K;
    if (pl.frame / K != b * G + s) { xlog(p, X264_LOG_ERROR, "x264_encoder_encode: GOP slots: picture %d was planned outside its GOP's turn (the GOPs of the stream are not closed and %d pictures long)\n", pl.frame, K); failed = true; return -1; }
    if (r == 0) gb_next = 0;
    DevCtx &dc = devs[(size_t)(s % D())];
    const size_t l = (size_t)(s / D()), row = (size_t)c.nmb * 4;
    Rec &rec = recs[(size_t)s * K + cpos];
    rec.type = pl.type; rec.disp = t; rec.qp = pl.qp; rec.qpm = pl.qpm; rec.direct_temporal = pl.direct_temporal;
    const void *rows[3] = { pl.d_offsets, pl.d_mvs[0], pl.d_mvs[1] };
    bool ok = x264gpu_memcpy_d2d(dc.d_ring + ((size_t)t * dc.nsl + l) * insz, pl.d_src, insz, nullptr) == X264GPU_OK;
    for (int a = 0; a < 3 && ok; a++) {
        rec.have[a] = rows[a] != nullptr;
        if (rows[a] && !dc.d_plan[a]) { xlog(p, X264_LOG_ERROR, "x264_encoder_encode: GOP slots: a picture was planned with rows its plan store was not opened for\n"); failed = true; return -1; }
        if (rows[a]) ok = x264gpu_memcpy_d2d(dc.d_plan[a] + ((size_t)cpos * dc.nsl + l) * row, rows[a], row, nullptr) == X264GPU_OK;
    }
    // (the copies run on the caller's device's stream; a slot on another device is coded on that device's: they are complete before it starts.  On the caller's own
    //  device the position's call runs behind them on the same stream; the lookahead reuses its arrays on that stream too)
    if (ok && dc.dev != c.device) ok = x264gpu_stream_sync(nullptr) == X264GPU_OK;
    if (!ok) { xlog(p, X264_LOG_ERROR, "x264_encoder_encode: upload failed: %s\n", x264gpu_last_error()); return -1; }
    submitted++;
    const bool full_gops = cpos < (int)gorder.size() && gorder[(size_t)cpos].first == t && gorder[(size_t)cpos].second == pl.type;
    if (s == G - 1 && full_gops && cpos == gb_next) {
        if (code_position_b((int)b, cpos, 0, G, gorder, gdpb) < 0) return -1;
        gb_next++;
        next_pos = cpos + 1 == K ? 0 : cpos + 1;
    } else if (!pool.empty()) join_pool();
    drain_coded();
    return 0;
}

// codes what the partly gathered batch holds, position by position, with the slots that have that position; later calls only drain
int GopSlots::flush()
{
    const int G = c.G, K = c.keyint;
    const long per_batch = (long)G * K;
    if (failed) return -1;
    const long i = submitted, b = i == 0 ? 0 : (i - 1) / per_batch, r = i - b * per_batch;    // r pictures in the last batch
    if (!flushed && r > 0 && !(r == per_batch && next_pos == 0)) {
        const int full = (int)(r / K), part = (int)(r % K);            // `full` complete GOPs, then `part` pictures
        if (gopb) {
            // the complete GOPs finish their plan in lock-step; then the stream's last, shorter GOP alone: its own coding order on a DPB model of its own,
            // from its IDR picture on (what the lock-step rounds coded of it while it was the batch's last slot is coded again: its tail differs)
            const bool last_ran = full == G - 1 && part > 0;          // (the partial GOP sat in the last slot: the rounds so far included it)
            if (!last_ran) gb_next = 0;                               // the last slot never delivered: nothing of this batch has been coded yet
            if (full > 0)
                for (int cpos = gb_next; cpos < K; cpos++)
                    if (code_position_b((int)b, cpos, 0, full, gorder, gdpb) < 0) return -1;
            if (part > 0) {
                join_pool();
                GopDpb gp;
                gp.dpb.configure(p->i_frame_reference, c.bframes, c.bpyramid, c.log2_max_frame_num, c.weightp);
                std::vector<std::pair<int, int>> po = gop_coding_order(part, c.bframes, c.bpyramid);
                // (quantisers planned ahead: the order the plan pass took, which is what the serial session codes)
                if (c.planned) for (int cpos = 0; cpos < part; cpos++) { const Rec &r = recs[(size_t)full * K + cpos]; po[(size_t)cpos] = { r.disp, r.type }; }
                for (int cpos = 0; cpos < part; cpos++) slot_have[(size_t)full * K + cpos] = 0;
                for (int cpos = 0; cpos < part; cpos++)
                    if (code_position_b((int)b, cpos, full, 1, po, gp) < 0) return -1;
            }
            gb_next = 0;
        } else
            for (int t = next_pos; t < K; t++) {
                const int nslots = full + (t < part ? 1 : 0);
                if (nslots <= 0) break;
                if (code_position((int)b, t, nslots) < 0) return -1;
            }
        next_pos = 0;
    }
    flushed = true;
    join_pool();
    drain_coded();
    return 0;
}

int GopSlots::recon(int slot, uint8_t *i420_out)
{
    if (slot < 0 || slot >= c.G || devs.empty()) return -1;
    join_pool();
    DevCtx &dc = devs[(size_t)(slot % D())];
    uint8_t *d = nullptr;
    int rc = D() > 1 ? x264gpu_set_device(dc.dev) : X264GPU_OK;
    if (rc == X264GPU_OK) rc = x264gpu_malloc((void **)&d, insz);
    if (rc == X264GPU_OK) rc = dc.solo.empty() ? x264gpu_encoder_get_recon(dc.gpu, slot / D(), d, nullptr) : x264gpu_encoder_get_recon(dc.solo[(size_t)(slot / D())], 0, d, nullptr);
    if (rc == X264GPU_OK) rc = x264gpu_memcpy_d2h(i420_out, d, insz, nullptr);
    if (d) x264gpu_free(d);
    if (D() > 1) (void)x264gpu_set_device(c.device);
    return rc == X264GPU_OK ? 0 : -1;
}

bool GopSlots::pop(Coded &cd)
{
    if (ready.empty()) return false;
    cd = std::move(ready.front());
    ready.pop_front();
    cd.index = emitted++;
    if (!gopb) { cd.pts = pts.front(); pts.pop_front(); }
    return true;
}

}  // namespace x264host

// batch.cpp — the cross-session batcher (batch.hpp): the group, the registry of groups, a round's launch, the members' downloads.
// Lock order: the registry's lock before a group's.  A round is run by the member whose submit (or whose leave) completes it, under the group's lock; an
// overlapping group that awaits its rounds releases the lock while it waits (running: nobody starts another).  The helper threads sleep on the group's one
// condition variable; whoever changes what they look at (launched, closed, a session's hurry flag) notifies under the group's lock.
#include "batch.hpp"
#include "quality.hpp"
#include "noisereduction.hpp"
#include "siderows.hpp"
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>

namespace x264host {

struct BatchGroup {
    std::mutex m; std::condition_variable cv;
    x264gpu_config cfg; int N = 0, device = 0;
    x264gpu_encoder *gpu = nullptr; uint8_t *d_in = nullptr; x264gpu_mb *d_mb = nullptr; int16_t *d_lv = nullptr;
    // overlap: the records / levels of round k are downloaded and entropy-coded (by a helper thread of every session) WHILE round k + 1 runs: a second pair of
    // output buffers used in turn, a stream of the group's own for the downloads; every session hands its pictures back one call later
    bool overlap = false; x264gpu_mb *d_mb2 = nullptr; int16_t *d_lv2 = nullptr; void *dl_stream = nullptr;
    // ... and (async) the callers do not wait for the round either: it is QUEUED on the group's own compute stream behind the round before, an event behind it tells the
    // download of its results when it is done; the callers go on to copy in and upload their next pictures (on upload streams of their own) while the device works
    bool async = false; void *cs = nullptr, *ev[2] = { nullptr, nullptr };
    // the levels leave the device packed (x264gpu_pack_levels behind every round, in place): a member downloads its records, its index and the part of its levels that is kept
    // (~10 % at medium; dense, 2048 members x 7 MB a round were what the first rounds waited for: fresh pages of the download buffers, 15 GB a round over the link)
    bool pack = false; x264gpu_level_index *d_ix = nullptr, *d_ix2 = nullptr;
    int qflags = 0; x264gpu_quality *d_q = nullptr, *d_q2 = nullptr;          // --psnr / --ssim of the members (all alike): one statistic per stream behind every round, two buffers as d_mb / d_mb2
    // --nr of the members (one strength a group): per stream the offsets, the last round's statistics and the running state; the update is queued behind every round
    int nr = 0; x264gpu_nr_offsets *d_nr_off = nullptr; x264gpu_nr_sums *d_nr_pic = nullptr, *d_nr_state = nullptr;
    // the members' side inputs (Batch::SideInputs; side: which arrays the members' lookaheads produce, and what else they agree in): per member the pointers handed in
    // with this round's picture; per array two generations of the gathered [N][nmb] rows, used in turn as the output buffers are (round k + 2 is launched only after
    // every member has round k's results: nothing of round k reads its generation any more); two generations of the device table of [3][N] row pointers the gather
    // reads, with its host image; the "absent" row that stands in for a member without vectors (first entry 0x7fff: x264gpu_encoder_set_lowres_mvs); the event that
    // tells the compute stream where the default stream — the members' lookaheads — stood when the round was complete
    Batch::Side side; std::vector<Batch::SideInputs> side_in; std::vector<const void *> side_tab;
    uint8_t *d_side[3][2] = { { nullptr, nullptr }, { nullptr, nullptr }, { nullptr, nullptr } }; const void **d_side_tab[2] = { nullptr, nullptr };
    int16_t *d_mv_absent = nullptr; void *ev_side = nullptr;
    std::vector<void *> up_streams;          // the members' uploads: a handful of streams dealt round-robin (a stream per member was 0.7 ms to create and 0.6 ms to destroy, x 2048, serialised in the runtime)
    long ev_round[2] = { 0, 0 }, ev_done[2] = { 0, 0 }; bool ev_waiting[2] = { false, false }; std::string ev_err;      // per buffer pair: the round recorded behind it (1-based), the last one known complete, a member is waiting for the event
    long launched = 0;            // rounds whose kernels have been issued: the helper threads start entropy coding round k once round k + 1 is on the device (or when asked to hurry),
                                  // so that the host cores are the callers' while the next pictures are uploaded and submitted
    bool running = false;         // a round is being waited for with the group's lock released (overlap): nobody starts another
    int leaving = 0; bool orphaned = false;      // Batch::leave: leavers between "decided to run the round" and "ran it"; the last member left meanwhile (the leaver destroys the group)
    size_t insz = 0, nmb = 0;
    std::vector<char> member, arrived; int joined = 0, active = 0, n_arrived = 0;
    std::vector<x264gpu_pic> pics; long round = 0; int round_rc = 0; std::string err;
    bool closed = false;          // a member left: no more joiners (Batch::leave)
    // X264GPU_BATCH_TIMING=1: where the members' threads spent their time, summed over members (printed when the group goes): waiting for a round's event,
    // downloading records / levels, waiting for the next round's launch before the slices are written, writing them, waiting in submit for the round to fill,
    // joining the helper thread
    std::atomic<long> t_us[6] = {};
    std::atomic<long> r_dl[64] = {}, r_sl[64] = {}, r_dl_first[64] = {}, r_dl_last[64] = {};          // per round: download / slice seconds summed over the members; when the first / last download ended
    std::vector<long> tl_launch, tl_done, tl_host;          // ... and per round: issued, its event seen, its results on the host (microseconds; the first launch = 0)
    bool timing = getenv("X264GPU_BATCH_TIMING") != nullptr;
};

namespace {

inline long us_now() { return (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
std::mutex g_batch_mu;
std::vector<BatchGroup *> g_batch_groups;

void batch_destroy(BatchGroup *g)
{
    const long t_destroy0 = g->timing ? us_now() : 0;
    struct Tm { BatchGroup *g; long t0; bool on; ~Tm() { if (on) fprintf(stderr, "x264gpu batch: the group's device memory and streams took %.2f s to release\n", (us_now() - t0) / 1e6); } } tm{ g, t_destroy0, g->timing };
    if (g->timing)
        fprintf(stderr, "x264gpu batch timing, seconds summed over %d members: event wait %.1f, download %.1f, wait for the next launch %.1f, slices %.1f, submit wait %.1f, join of the helper %.1f\n", g->N,
                g->t_us[0] / 1e6, g->t_us[1] / 1e6, g->t_us[2] / 1e6, g->t_us[3] / 1e6, g->t_us[4] / 1e6, g->t_us[5] / 1e6);
    if (g->timing && !g->tl_launch.empty()) {
        fprintf(stderr, "x264gpu batch rounds (s from the first launch): issued / event seen / results on the host:");
        for (size_t i = 0; i < g->tl_launch.size(); i++)
            fprintf(stderr, "  %zu: %.2f / %.2f / %.2f", i, (g->tl_launch[i] - g->tl_launch[0]) / 1e6, i < g->tl_done.size() ? (g->tl_done[i] - g->tl_launch[0]) / 1e6 : -1., i < g->tl_host.size() ? (g->tl_host[i] - g->tl_launch[0]) / 1e6 : -1.);
        fprintf(stderr, "\n");
        fprintf(stderr, "x264gpu batch rounds: download s per member / slices s per member / first .. last download done (s from the first launch):");
        for (size_t i = 0; i < g->tl_launch.size() && i < 64; i++)
            fprintf(stderr, "  %zu: %.2f / %.2f / %.2f .. %.2f", i, g->r_dl[i] / 1e6 / g->N, g->r_sl[i] / 1e6 / g->N, (g->r_dl_first[i] - g->tl_launch[0]) / 1e6, (g->r_dl_last[i] - g->tl_launch[0]) / 1e6);
        fprintf(stderr, "\n");
    }
    // nothing of the group's is released while one of its streams may still work on it: the last round (a leaver's, or one a failed member never downloaded),
    // the downloads and the uploads drain first; then the encoder and the buffers go, then the events and the streams
    if (g->cs) x264gpu_stream_sync(g->cs);
    if (g->dl_stream) x264gpu_stream_sync(g->dl_stream);
    for (void *st : g->up_streams) x264gpu_stream_sync(st);
    if (g->gpu) x264gpu_encoder_destroy(g->gpu);
    if (g->d_in) x264gpu_free(g->d_in);
    if (g->d_mb) x264gpu_free(g->d_mb);
    if (g->d_lv) x264gpu_free(g->d_lv);
    if (g->d_mb2) x264gpu_free(g->d_mb2);
    if (g->d_lv2) x264gpu_free(g->d_lv2);
    if (g->d_ix) x264gpu_free(g->d_ix);
    if (g->d_ix2) x264gpu_free(g->d_ix2);
    if (g->d_q) x264gpu_free(g->d_q);
    if (g->d_q2) x264gpu_free(g->d_q2);
    if (g->d_nr_off) x264gpu_free(g->d_nr_off);
    if (g->d_nr_pic) x264gpu_free(g->d_nr_pic);
    if (g->d_nr_state) x264gpu_free(g->d_nr_state);
    for (int a = 0; a < 3; a++) for (int i = 0; i < 2; i++) if (g->d_side[a][i]) x264gpu_free(g->d_side[a][i]);
    for (int i = 0; i < 2; i++) if (g->d_side_tab[i]) x264gpu_free((void *)g->d_side_tab[i]);
    if (g->d_mv_absent) x264gpu_free(g->d_mv_absent);
    if (g->ev_side) x264gpu_event_destroy(g->ev_side);
    for (int i = 0; i < 2; i++) if (g->ev[i]) x264gpu_event_destroy(g->ev[i]);
    if (g->dl_stream) x264gpu_stream_destroy(g->dl_stream);
    for (void *st : g->up_streams) x264gpu_stream_destroy(st);
    if (g->cs) x264gpu_stream_destroy(g->cs);
    delete g;
}

// in front of a round of a group whose members have lookaheads: their quantiser offsets and low-resolution vectors of this round's pictures become the device
// encoder's [N][nmb] arrays — on the stream the round runs on, behind what the members' lookaheads wrote on the default stream.  first: a member that arrived
// (a stream whose session has gone takes its rows: coded along, thrown away).  false: g->err says why
bool batch_side_inputs(BatchGroup *g, int first)
{
    const size_t N = (size_t)g->N, row = g->nmb * 4;          // a float, or a vector of two int16, a macroblock
    const int gen = (int)(g->round & 1);
    void *const st = g->async ? g->cs : nullptr;
    bool any[3] = { false, false, false };
    for (size_t s = 0; s < N; s++) {
        const Batch::SideInputs &in = g->side_in[g->arrived[s] ? s : (size_t)first];
        const void *p[3] = { in.d_offsets, in.d_mvs0, in.d_mvs1 };
        for (int a = 0; a < 3; a++) { g->side_tab[(size_t)a * N + s] = p[a]; any[a] = any[a] || p[a]; }
    }
    for (int a = 0; a < 3; a++) if (any[a] && !g->d_side[a][gen]) { g->err = "X264GPU_BATCH: a session handed in side inputs its group was not opened for"; return false; }
    // (a member without vectors among members with them: "absent" is a row that says so, not a row of zero vectors)
    for (int a = 1; a < 3; a++) if (any[a]) for (size_t s = 0; s < N; s++) if (!g->side_tab[(size_t)a * N + s]) g->side_tab[(size_t)a * N + s] = g->d_mv_absent;
    bool ok = true;
    if (any[0] || any[1] || any[2]) {
        if (g->async) ok = x264gpu_event_record(g->ev_side, nullptr) == X264GPU_OK && x264gpu_stream_wait_event(st, g->ev_side) == X264GPU_OK;
        // (the table goes up on an upload stream, not on the compute stream, which still runs the round before)
        uint8_t *const dst[3] = { g->d_side[0][gen], g->d_side[1][gen], g->d_side[2][gen] };
        ok = ok && side_rows_gather(g->side_tab.data(), any, g->d_side_tab[gen], dst, N, row, st, g->up_streams.empty() ? nullptr : g->up_streams[0]);
    }
    ok = ok && x264gpu_encoder_set_mb_qp_offsets(g->gpu, any[0] ? (const float *)g->d_side[0][gen] : nullptr) == X264GPU_OK &&
         x264gpu_encoder_set_lowres_mvs(g->gpu, any[1] ? (const int16_t *)g->d_side[1][gen] : nullptr) == X264GPU_OK &&
         x264gpu_encoder_set_lowres_mvs1(g->gpu, any[2] ? (const int16_t *)g->d_side[2][gen] : nullptr) == X264GPU_OK;
    if (!ok) g->err = x264gpu_last_error();
    return ok;
}

// the launch of a complete round; g->m is held through lk (released while an overlapping group waits for its kernels)
void batch_run_round(BatchGroup *g, std::unique_lock<std::mutex> &lk)
{
    int first = -1;
    for (int s = 0; s < g->N; s++) if (g->arrived[(size_t)s]) { first = s; break; }
    g->round_rc = 0; g->err.clear();
    if (first >= 0) {
        for (int s = 0; s < g->N; s++) {
            if (!g->arrived[(size_t)s]) { g->pics[(size_t)s] = g->pics[(size_t)first]; continue; }      // a stream whose session has gone: coded along, thrown away
            const x264gpu_pic &a = g->pics[(size_t)s], &b = g->pics[(size_t)first];
            if (a.slice_type != b.slice_type || a.poc != b.poc || a.dst != b.dst || a.keep != b.keep || a.nref[0] != b.nref[0] || a.nref[1] != b.nref[1] ||
                memcmp(a.slot, b.slot, sizeof(a.slot)) || a.blind_dupe != b.blind_dupe) { g->round_rc = -1; g->err = "the sessions of a batch must submit pictures of the same structure (same picture count, keyint, bframes, forced types)"; }
        }
        const bool second = g->overlap && (g->round & 1);          // the output buffers of this round (the other pair may still be downloading)
        if (!g->round_rc && (g->side.offsets || g->side.mvs) && !batch_side_inputs(g, first)) g->round_rc = -1;
        if (!g->round_rc && x264gpu_encode_pictures(g->gpu, g->d_in, g->pics.data(), second ? g->d_mb2 : g->d_mb, second ? g->d_lv2 : g->d_lv, g->async ? g->cs : nullptr) != X264GPU_OK) { g->round_rc = -1; g->err = x264gpu_last_error(); }
        // --nr: a batch session's picture is accepted as it is coded (no VBV in a group): every stream's statistics join its state, its next offsets follow, in front of the next round
        if (!g->round_rc && g->nr && nr_update_queue(g->d_nr_off, g->d_nr_state, g->d_nr_pic, g->N, g->nr, g->async ? g->cs : nullptr) != X264GPU_OK) { g->round_rc = -1; g->err = x264gpu_last_error(); }
        if (!g->round_rc && g->qflags && quality_queue(g->gpu, g->qflags, second ? g->d_q2 : g->d_q, g->async ? g->cs : nullptr) != X264GPU_OK) { g->round_rc = -1; g->err = x264gpu_last_error(); }
        if (!g->round_rc && g->pack && x264gpu_pack_levels(second ? g->d_lv2 : g->d_lv, g->N, (int)g->nmb, second ? g->d_ix2 : g->d_ix, nullptr, g->cs) != X264GPU_OK) { g->round_rc = -1; g->err = x264gpu_last_error(); }
        if (!g->round_rc && g->async) {
            // queued, not awaited: the event behind the round is what its downloads wait for (Batch::download)
            if (x264gpu_event_record(g->ev[second ? 1 : 0], g->cs) != X264GPU_OK) { g->round_rc = -1; g->err = x264gpu_last_error(); }
            g->launched++;
            if (g->timing) g->tl_launch.push_back(us_now());
            g->ev_round[second ? 1 : 0] = g->round + 1;
        } else
        // overlap: the downloads run on the group's own stream, which does not wait for the default one: the round must be complete before anyone is told
        if (!g->round_rc && g->overlap) {
            g->launched++; g->running = true;
            g->cv.notify_all();          // the helper threads of the round before: the device is busy again, the host cores are theirs
            lk.unlock();
            const bool ok = x264gpu_stream_sync(nullptr) == X264GPU_OK;
            std::string e = ok ? std::string() : std::string(x264gpu_last_error());
            lk.lock();
            g->running = false;
            if (!ok) { g->round_rc = -1; g->err = e; }
        }
    }
    g->round++; g->n_arrived = 0;
    std::fill(g->arrived.begin(), g->arrived.end(), 0);
    g->cv.notify_all();
}

}  // namespace

bool Batch::join(const x264gpu_config &cfg1, int N, size_t insz, size_t nmb, int qflags, int nr, bool nr_any, const Side &side)
{
    std::lock_guard<std::mutex> lk(g_batch_mu);
    int dev = 0;
    (void)x264gpu_get_device(&dev);
    for (BatchGroup *og : g_batch_groups) {
        x264gpu_config a = og->cfg, b = cfg1;
        a.streams = b.streams = 0;
        if (og->N == N && og->device == dev && og->joined < N && !og->closed && og->qflags == qflags && og->nr == nr &&
            og->side.offsets == side.offsets && og->side.mvs == side.mvs && og->side.key == side.key && !memcmp(&a, &b, sizeof(a))) {
            std::lock_guard<std::mutex> lg(og->m);
            g = og; s = og->joined++; og->active++; og->member[(size_t)s] = 1;
            og->cv.notify_all();
            break;
        }
    }
    if (!g) {
        BatchGroup *ng = new BatchGroup();
        ng->cfg = cfg1; ng->cfg.streams = N; ng->N = N; ng->device = dev; ng->insz = insz; ng->nmb = nmb; ng->qflags = qflags; ng->nr = nr; ng->side = side;
        ng->member.assign((size_t)N, 0); ng->arrived.assign((size_t)N, 0); ng->pics.resize((size_t)N); ng->side_in.resize((size_t)N); ng->side_tab.assign(3 * (size_t)N, nullptr);
        if (x264gpu_encoder_create(&ng->gpu, &ng->cfg) != X264GPU_OK ||
            x264gpu_malloc((void **)&ng->d_in, (size_t)N * insz) != X264GPU_OK ||
            x264gpu_malloc((void **)&ng->d_mb, (size_t)N * nmb * sizeof(x264gpu_mb)) != X264GPU_OK ||
            x264gpu_malloc((void **)&ng->d_lv, (size_t)N * nmb * X264GPU_MB_LEVELS * sizeof(int16_t)) != X264GPU_OK ||
            (qflags && (x264gpu_malloc((void **)&ng->d_q, (size_t)N * sizeof(x264gpu_quality)) != X264GPU_OK || x264gpu_malloc((void **)&ng->d_q2, (size_t)N * sizeof(x264gpu_quality)) != X264GPU_OK))) { batch_destroy(ng); return false; }
        if (nr && (x264gpu_malloc((void **)&ng->d_nr_off, (size_t)N * sizeof(x264gpu_nr_offsets)) != X264GPU_OK || x264gpu_malloc((void **)&ng->d_nr_pic, (size_t)N * sizeof(x264gpu_nr_sums)) != X264GPU_OK ||
                   x264gpu_malloc((void **)&ng->d_nr_state, (size_t)N * sizeof(x264gpu_nr_sums)) != X264GPU_OK ||
                   x264gpu_memset(ng->d_nr_off, 0, (size_t)N * sizeof(x264gpu_nr_offsets), nullptr) != X264GPU_OK || x264gpu_memset(ng->d_nr_pic, 0, (size_t)N * sizeof(x264gpu_nr_sums), nullptr) != X264GPU_OK ||
                   x264gpu_memset(ng->d_nr_state, 0, (size_t)N * sizeof(x264gpu_nr_sums), nullptr) != X264GPU_OK || x264gpu_stream_sync(nullptr) != X264GPU_OK ||
                   nr_set(ng->gpu, ng->d_nr_off, ng->d_nr_pic, nr_any) != X264GPU_OK)) { batch_destroy(ng); return false; }
        if (side.offsets || side.mvs) {
            // the gathered arrays and the tables of row pointers, two generations each; the vectors' "absent" row
            const size_t rows = (size_t)N * nmb * 4;
            bool ok = x264gpu_event_create(&ng->ev_side) == X264GPU_OK;
            for (int i = 0; i < 2 && ok; i++) {
                ok = x264gpu_malloc((void **)&ng->d_side_tab[i], 3 * (size_t)N * sizeof(void *)) == X264GPU_OK && (!side.offsets || x264gpu_malloc((void **)&ng->d_side[0][i], rows) == X264GPU_OK) &&
                     (!side.mvs || (x264gpu_malloc((void **)&ng->d_side[1][i], rows) == X264GPU_OK && x264gpu_malloc((void **)&ng->d_side[2][i], rows) == X264GPU_OK));
            }
            ok = ok && (!side.mvs || (ng->d_mv_absent = side_rows_absent(nmb)) != nullptr);
            if (!ok) { batch_destroy(ng); return false; }
        }
        const char *oe = getenv("X264GPU_BATCH_OVERLAP");
        if (!(oe && oe[0] == '0') && !getenv("X264GPU_DUMP_RECORDS") &&
            x264gpu_malloc((void **)&ng->d_mb2, (size_t)N * nmb * sizeof(x264gpu_mb)) == X264GPU_OK &&
            x264gpu_malloc((void **)&ng->d_lv2, (size_t)N * nmb * X264GPU_MB_LEVELS * sizeof(int16_t)) == X264GPU_OK && x264gpu_stream_create(&ng->dl_stream) == X264GPU_OK) ng->overlap = true;
        const char *ae = getenv("X264GPU_BATCH_ASYNC");
        if (ng->overlap && !(ae && ae[0] == '0') && x264gpu_stream_create(&ng->cs) == X264GPU_OK && x264gpu_event_create(&ng->ev[0]) == X264GPU_OK && x264gpu_event_create(&ng->ev[1]) == X264GPU_OK) ng->async = true;
        if (ng->async && !getenv("X264GPU_BATCH_DENSE") && x264gpu_malloc((void **)&ng->d_ix, (size_t)N * nmb * sizeof(x264gpu_level_index)) == X264GPU_OK &&
            x264gpu_malloc((void **)&ng->d_ix2, (size_t)N * nmb * sizeof(x264gpu_level_index)) == X264GPU_OK) ng->pack = true;
        if (ng->async) for (int i = 0; i < 16 && i < N; i++) { void *st = nullptr; if (x264gpu_stream_create(&st) == X264GPU_OK) ng->up_streams.push_back(st); else break; }
        ng->joined = 1; ng->active = 1; ng->member[0] = 1;
        g_batch_groups.push_back(ng);
        g = ng; s = 0;
    }
    up = g->async && !g->up_streams.empty() ? g->up_streams[(size_t)s % g->up_streams.size()] : nullptr;
    return true;
}

int Batch::size() const { return g ? g->N : 0; }
bool Batch::carries_offsets() const { return g && g->side.offsets; }
bool Batch::carries_mvs() const { return g && g->side.mvs; }
bool Batch::overlap() const { return g && g->overlap; }
bool Batch::queued() const { return g && g->async; }
bool Batch::packed() const { return g && g->pack; }

int Batch::submit(const uint8_t *d_src, const x264gpu_pic &pic, const SideInputs &side, int *buf, std::string &err)
{
    // (async: on the group's compute stream, i.e. behind the round before — which may still be reading d_in — and in front of this round's launch)
    if (x264gpu_memcpy_d2d(g->d_in + (size_t)s * g->insz, d_src, g->insz, g->async ? g->cs : nullptr) != X264GPU_OK) { err = x264gpu_last_error(); return -1; }
    std::unique_lock<std::mutex> lk(g->m);
    // every member must have been opened before the first picture is coded: a late joiner would be a picture behind for good
    if (!g->cv.wait_for(lk, std::chrono::seconds(60), [&] { return g->joined == g->N; })) { err = "X264GPU_BATCH: fewer sessions were opened than the batch size"; return -1; }
    g->pics[(size_t)s] = pic; g->side_in[(size_t)s] = side; g->arrived[(size_t)s] = 1; g->n_arrived++;
    const long my_round = g->round;
    *buf = g->overlap ? (int)(my_round & 1) : 0;
    const long t0 = g->timing ? us_now() : 0;
    struct Acc { BatchGroup *g; long t0; ~Acc() { if (g->timing) g->t_us[4] += us_now() - t0; } } acc{ g, t0 };
    if (g->n_arrived >= g->active && !g->running) batch_run_round(g, lk);
    else if (!g->cv.wait_for(lk, std::chrono::seconds(600), [&] { return g->round != my_round; })) {
        // a member neither submitted its picture nor closed: give up on this session (the others keep waiting for it, or for its close)
        g->arrived[(size_t)s] = 0; g->n_arrived--;
        err = "X264GPU_BATCH: another session of the batch stopped submitting pictures";
        return -1;
    }
    if (g->round_rc) { err = g->err; return -1; }
    return 0;
}

int Batch::download(int buf, x264gpu_mb *h_mb, int16_t *h_lv, std::string &err, x264gpu_level_index *h_ix, x264gpu_quality *h_q)
{
    const x264gpu_mb *dm = buf ? g->d_mb2 : g->d_mb; const int16_t *dl = buf ? g->d_lv2 : g->d_lv;
    // (async groups: the members' downloads are dealt to the group's sixteen upload / download streams)
    void *st = g->overlap ? (g->up_streams.empty() ? g->dl_stream : g->up_streams[(size_t)s % g->up_streams.size()]) : nullptr;
    const long t0 = g->timing ? us_now() : 0;
    if (g->async) {
        // ONE thread waits for the round's event, the other members sleep on the group's condition variable (2048 helper threads in hipEventSynchronize would
        // take the host's cores from the callers that are copying in and uploading the next pictures)
        std::unique_lock<std::mutex> lk(g->m);
        const long want = g->ev_round[buf ? 1 : 0];          // the round recorded behind this buffer pair (it cannot be re-recorded before every member has this round's results)
        while (g->ev_done[buf ? 1 : 0] < want) {
            if (!g->ev_waiting[buf ? 1 : 0]) {
                g->ev_waiting[buf ? 1 : 0] = true;
                lk.unlock();
                const bool ok = x264gpu_event_sync(g->ev[buf ? 1 : 0]) == X264GPU_OK;
                const long t_ev = g->timing ? us_now() : 0;
                const std::string e = ok ? std::string() : std::string(x264gpu_last_error());
                lk.lock();
                if (g->timing) { g->tl_done.push_back(t_ev); g->tl_host.push_back(us_now()); }
                g->ev_waiting[buf ? 1 : 0] = false;
                if (!ok) { g->ev_err = e; g->ev_done[buf ? 1 : 0] = want; g->cv.notify_all(); err = e; return -1; }
                g->ev_done[buf ? 1 : 0] = want;
                g->cv.notify_all();
            } else g->cv.wait(lk);
        }
        if (!g->ev_err.empty()) { err = g->ev_err; return -1; }
    }
    const long t1 = g->timing ? us_now() : 0;
    const long rnd = g->async ? g->ev_round[buf ? 1 : 0] - 1 : 0;
    struct Acc { BatchGroup *g; long t0, t1, rnd; ~Acc() { if (g->timing) { const long t2 = us_now(); g->t_us[0] += t1 - t0; g->t_us[1] += t2 - t1;
        if (rnd >= 0 && rnd < 64) { g->r_dl[rnd] += t2 - t1; long f = g->r_dl_first[rnd].load(); while ((f == 0 || t2 < f) && !g->r_dl_first[rnd].compare_exchange_weak(f, t2)) {} long l = g->r_dl_last[rnd].load(); while (t2 > l && !g->r_dl_last[rnd].compare_exchange_weak(l, t2)) {} } } } } acc{ g, t0, t1, rnd };
    if (g->qflags && h_q && x264gpu_memcpy_d2h(h_q, (buf ? g->d_q2 : g->d_q) + s, sizeof(x264gpu_quality), st) != X264GPU_OK) { err = x264gpu_last_error(); return -1; }
    if (g->pack) {
        if (!h_ix) { err = "X264GPU_BATCH: the group's levels are packed"; return -1; }
        const x264gpu_level_index *di = (buf ? g->d_ix2 : g->d_ix) + (size_t)s * g->nmb;
        if (x264gpu_memcpy_d2h(h_mb, dm + (size_t)s * g->nmb, g->nmb * sizeof(x264gpu_mb), st) != X264GPU_OK ||
            x264gpu_memcpy_d2h(h_ix, di, g->nmb * sizeof(x264gpu_level_index), st) != X264GPU_OK) { err = x264gpu_last_error(); return -1; }
        const size_t kept = ((size_t)h_ix[g->nmb - 1].at + (size_t)__builtin_popcount(h_ix[g->nmb - 1].groups)) * 16;          // levels
        if (kept > g->nmb * (size_t)X264GPU_MB_LEVELS) { err = "X264GPU_BATCH: level index out of range"; return -1; }
        if (kept && x264gpu_memcpy_d2h(h_lv, dl + (size_t)s * g->nmb * X264GPU_MB_LEVELS, kept * sizeof(int16_t), st) != X264GPU_OK) { err = x264gpu_last_error(); return -1; }
        return 0;
    }
    if (x264gpu_memcpy_d2h(h_mb, dm + (size_t)s * g->nmb, g->nmb * sizeof(x264gpu_mb), st) != X264GPU_OK ||
        x264gpu_memcpy_d2h(h_lv, dl + (size_t)s * g->nmb * X264GPU_MB_LEVELS, g->nmb * X264GPU_MB_LEVELS * sizeof(int16_t), st) != X264GPU_OK) { err = x264gpu_last_error(); return -1; }
    return 0;
}

int Batch::nr_offsets(uint16_t out[3][64])
{
    memset(out, 0, 3 * 64 * sizeof(uint16_t));
    if (!g || !g->nr) return -1;
    // (the update is queued on the stream the rounds run on: wait for it, then for the copy)
    void *st = g->async ? g->cs : nullptr;
    if (x264gpu_stream_sync(st) != X264GPU_OK || x264gpu_memcpy_d2h(out, g->d_nr_off + s, sizeof(x264gpu_nr_offsets), st) != X264GPU_OK || x264gpu_stream_sync(st) != X264GPU_OK) return -1;
    return 0;
}

long Batch::launched()
{
    std::lock_guard<std::mutex> lg(g->m);
    return g->launched;
}

void Batch::wait_launched(long after, const std::atomic<bool> &hurry)
{
    const long t0 = g->timing ? us_now() : 0;
    {
        std::unique_lock<std::mutex> lk(g->m);
        g->cv.wait_for(lk, std::chrono::seconds(30), [&] { return g->launched > after || hurry.load() || g->closed; });
    }
    if (g->timing) g->t_us[2] += us_now() - t0;
}

void Batch::wake()
{
    if (!g) return;
    std::lock_guard<std::mutex> lg(g->m);
    g->cv.notify_all();
}

void Batch::timed(Span what, long round, const std::function<void()> &f)
{
    if (!g || !g->timing) { f(); return; }
    const long t0 = us_now();
    f();
    const long t = us_now() - t0;
    g->t_us[what == SLICES ? 3 : 5] += t;
    if (what == SLICES && round >= 1 && round <= 64) g->r_sl[round - 1] += t;
}

void Batch::leave()
{
    if (!g) return;
    BatchGroup *const grp = g;
    const int seat = s;
    g = nullptr; s = -1; up = nullptr;
    // the registry lock first (the order join takes them in): "last" is decided and the group unlisted under it, so that a joiner can
    // never be handed a group that is about to be destroyed; a group that lost a member takes no more joiners (closed), its seats stay empty
    // ... and ONLY that under it: the round the others were waiting for (a whole device launch plus downloads) runs after the registry lock is released,
    // under the group's own lock — every x264_encoder_open / close that touches the batcher would otherwise wait for a GPU round
    bool last, run = false;
    {
        std::lock_guard<std::mutex> reg(g_batch_mu);
        std::unique_lock<std::mutex> lk(grp->m);
        grp->member[(size_t)seat] = 0; grp->active--; grp->closed = true;
        last = grp->active == 0;
        run = !last && grp->n_arrived >= grp->active && grp->n_arrived > 0;      // the others were only waiting for this session
        if (run) grp->leaving++;          // keeps the group alive across the gap below: a member that times out and closes meanwhile must not destroy it under this thread
        if (last)
            for (size_t i = 0; i < g_batch_groups.size(); i++) if (g_batch_groups[i] == grp) { g_batch_groups.erase(g_batch_groups.begin() + (long)i); break; }
        if (last && grp->leaving > 0) { grp->orphaned = true; last = false; }          // the leaver still inside destroys it when it is done
    }
    if (run) {
        bool destroy = false;
        {
            std::unique_lock<std::mutex> lk(grp->m);
            if (grp->active > 0 && grp->n_arrived >= grp->active && grp->n_arrived > 0 && !grp->running) batch_run_round(grp, lk);
            grp->leaving--;
            destroy = grp->orphaned && grp->leaving == 0;
        }
        if (destroy) batch_destroy(grp);
    }
    if (last) batch_destroy(grp);
}

}  // namespace x264host

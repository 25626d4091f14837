// qprd.hip.h — x264's QP-RD (--subme 10, i_mbrd 3; mb_analyse_qp_rd): once a macroblock's type, partition, transform size, vectors and intra modes are
// final, neighbouring quantisers are tried for it and the one with the lowest RD cost is kept.  The walk is written ONCE, as a resumable state
// machine over plain integers: it is handed the cost and cbp_empty of the encode it asked for last and answers "code at w.q next" (QPRD_CODE), "flip
// the transform size and code at w.q" (QPRD_FLIP) or "done: w.bqp, w.flip" (QPRD_DONE).  The macroblock loop (k_mb.hip.h, the QPRD instantiations)
// drives it with candidate passes, the primitive x264gpu_qprd_walk (qprd_kernels.hip) with table lookups; tests/qprd_ref.py is its Python twin.
//
// libx264 is not among the sources this project was written against: what follows is a recollection.
//   origcost = bcost = cost(orig_qp); bqp = orig_qp; origcbp = !cbp_empty; last_tried = false
//   for direction in (origcbp ? [+1, -1] : [-1]):
//       threshold = psy; one more when the direction leads towards last_qp
//       failures = 0; prevcost = origcost; checked_qp = -1
//       if direction == -1 && !origcbp:           # nothing coded at orig_qp: jump down past the threshold at once
//           q = max(orig_qp - threshold - 1, qp_min); checked_cost, empty = cost(q)         # (not compared with bcost)
//           if empty: { if last_qp > q: last_tried = true; break }
//           checked_qp = q
//       q = orig_qp + direction
//       while qp_min <= q <= qp_max:
//           if q == last_qp: last_tried = true
//           if q == checked_qp: c = checked_cost                                             # (reused, and not compared with bcost)
//           else: c, empty = cost(q); if c < bcost: bcost, bqp = c, q
//           failures = c < prevcost ? 0 : failures + 1; prevcost = c                         # (a tie is a failure)
//           if failures > threshold: break
//           if direction == +1 && empty: break
//           q += direction
//   if !last_tried: c = cost(last_qp); if c < bcost: bcost, bqp = c, last_qp
//   if bqp != orig_qp && the transform size may be chosen: c = cost(bqp, other transform size); the flip stays unless c > bcost
// `empty` is the cbp_empty of the encode that ran LAST: after a reused checked_qp it is still that of the encode before.  Only the walk upwards reads
// it, and a walk upwards has no checked_qp (the jump belongs to the lone walk down of a macroblock with nothing coded), so the stale value never
// decides anything; the machine keeps it as x264 does all the same.
// Two rules that x264 never needs, because its rate control clips every macroblock's quantiser to [qp_min, qp_max] (here AQ and the lookahead's offsets clip to
// 1 .. 51 only): the walk CHOOSES inside the range only — a macroblock whose own quantiser lies outside is left alone (no encode is asked for), and a last_qp
// outside is not tried.
// cbp_empty: h->mb.cbp of the macroblock is 0 — no luma 8x8 block and no chroma coded, and no Intra_16x16 DC level (CABAC keeps the DC flags in there).
// The state is wave-uniform wherever its inputs are: the macroblock loop holds every field in a scalar register (uni()).
#pragma once

namespace x264gpu {

enum { QPRD_CODE = 0, QPRD_FLIP = 1, QPRD_DONE = 2 };
enum { QPRD_S_ORIG = 0, QPRD_S_JUMP = 1, QPRD_S_WALK = 2, QPRD_S_LAST = 3, QPRD_S_FLIP = 4 };
constexpr int QPRD_LOG_WORDS = 128, QPRD_LOG_MAX = 63;      // a log entry (x264gpu_encoder_set_qprd_log): 2 words + 63 samples of 2

struct QprdWalk {
    int st, orig, last, qmin, qmax, psy, t8ok;          // what the walk waits for; its inputs
    int di, dir, thr, fail, prev, chk_q, chk_c;         // the direction being walked
    int q, bcost, bqp, origcost;                        // the quantiser asked for; the best so far
    int origcbp, last_tried, empty, flip;
};

// -> QPRD_CODE: the first encode, at the macroblock's own quantiser (QPRD_DONE: that one lies outside the range, there is no walk)
__host__ __device__ __forceinline__ int qprd_start(QprdWalk &w, int orig_qp, int last_qp, int qp_min, int qp_max, int psy, int t8_eligible)
{
    w.st = QPRD_S_ORIG; w.orig = orig_qp; w.last = last_qp; w.qmin = qp_min; w.qmax = qp_max; w.psy = psy != 0; w.t8ok = t8_eligible != 0;
    w.di = -1; w.dir = 0; w.thr = 0; w.fail = 0; w.prev = 0; w.chk_q = -1; w.chk_c = 0;
    w.q = orig_qp; w.bcost = 0; w.bqp = orig_qp; w.origcost = 0; w.origcbp = 0; w.last_tried = 0; w.empty = 0; w.flip = 0;
    return orig_qp < qp_min || orig_qp > qp_max ? QPRD_DONE : QPRD_CODE;
}

// the end of one round of the while loop with cost c at w.q (fresh: an encode ran for it) -> the direction's loop ends
__host__ __device__ __forceinline__ bool qprd_tail(QprdWalk &w, int c, bool fresh)
{
    if (fresh && c < w.bcost) { w.bcost = c; w.bqp = w.q; }
    w.fail = c < w.prev ? 0 : w.fail + 1;
    w.prev = c;
    if (w.fail > w.thr) return true;
    if (w.dir == 1 && w.empty) return true;
    w.q += w.dir;
    return false;
}

// cost / cbp_empty of the encode asked for last -> the next action
__host__ __device__ __forceinline__ int qprd_step(QprdWalk &w, int cost, int cbp_empty)
{
    enum { OPEN, HEAD, DIRS_DONE, FLIPCHK };
    int pc = OPEN;
    if (w.st == QPRD_S_ORIG) {
        w.origcost = w.bcost = cost; w.bqp = w.orig; w.empty = cbp_empty != 0; w.origcbp = !w.empty; w.last_tried = 0; w.di = -1;
    } else if (w.st == QPRD_S_JUMP) {
        w.empty = cbp_empty != 0; w.chk_c = cost;
        if (w.empty) { if (w.last > w.q) w.last_tried = 1; pc = DIRS_DONE; }
        else { w.chk_q = w.q; w.q = w.orig + w.dir; pc = HEAD; }
    } else if (w.st == QPRD_S_WALK) {
        w.empty = cbp_empty != 0;
        pc = qprd_tail(w, cost, true) ? OPEN : HEAD;
    } else if (w.st == QPRD_S_LAST) {
        if (cost < w.bcost) { w.bcost = cost; w.bqp = w.last; }
        pc = FLIPCHK;
    } else {
        w.flip = !(cost > w.bcost);
        w.q = w.bqp;
        return QPRD_DONE;
    }
    for (;;) {
        if (pc == OPEN) {
            w.di++;
            if (w.di >= (w.origcbp ? 2 : 1)) { pc = DIRS_DONE; continue; }
            w.dir = w.origcbp && w.di == 0 ? 1 : -1;
            w.thr = w.psy + (((w.last < w.orig && w.dir == -1) || (w.last > w.orig && w.dir == 1)) ? 1 : 0);
            w.fail = 0; w.prev = w.origcost; w.chk_q = -1;
            if (w.dir == -1 && !w.origcbp) {
                w.q = w.orig - w.thr - 1 > w.qmin ? w.orig - w.thr - 1 : w.qmin;
                w.st = QPRD_S_JUMP;
                return QPRD_CODE;
            }
            w.q = w.orig + w.dir;
            pc = HEAD;
        } else if (pc == HEAD) {
            if (w.q < w.qmin || w.q > w.qmax) { pc = OPEN; continue; }
            if (w.q == w.last) w.last_tried = 1;
            if (w.q != w.chk_q) { w.st = QPRD_S_WALK; return QPRD_CODE; }
            if (qprd_tail(w, w.chk_c, false)) pc = OPEN;
        } else if (pc == DIRS_DONE) {
            if (!w.last_tried && w.last >= w.qmin && w.last <= w.qmax) { w.q = w.last; w.st = QPRD_S_LAST; return QPRD_CODE; }
            pc = FLIPCHK;
        } else {
            w.q = w.bqp;
            if (w.bqp != w.orig && w.t8ok) { w.st = QPRD_S_FLIP; return QPRD_FLIP; }
            w.flip = 0;
            return QPRD_DONE;
        }
    }
}

}  // namespace x264gpu

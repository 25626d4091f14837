// slicetype.cpp — the slice-type unit (slicetype.hpp): x264_slicetype_analyse / x264_slicetype_decide on the device's frame costs
#include "slicetype.hpp"
#include <math.h>

namespace x264host {

enum { ST_AUTO = 0, ST_IDR, ST_I, ST_P, ST_BREF, ST_B };          // Frame::type
constexpr int ST_PATH_MAX = 96;
static bool is_b(int t) { return t == ST_B || t == ST_BREF; }
struct SliceType::Window {
    SliceType &s; const RateControl &rc; std::vector<Frame *> f;
    Window(SliceType &s_, const RateControl &rc_) : s(s_), rc(rc_) { f.push_back(&s.last_nonb); }
    Frame &fr(int i) const { return *f[(size_t)i]; }
    bool isb(int i) const { return is_b(fr(i).type); }
    int frame_cost(int p0, int p1, int b);
    bool scenecut_internal(int p0, int p1);
    bool scenecut(int p0, int p1, bool real, int num_frames, int i_max_search);
    void macroblock_tree(int num_frames, bool b_intra);
    uint64_t path_cost(const char *path0, uint64_t threshold);
    void path(int length, char (*best_paths)[ST_PATH_MAX + 1]);
    void vbv_lookahead(int num_frames, bool keyframe);
    void analyse(int framecnt, bool keyframe = false);
};

bool SliceType::open(x264_param_t &param, const RateControl &rc, const Setup &setup)
{
    p = &param; c = setup;
    weightp_fake = !c.weightp && c.mbtree && p->analyse.b_psy;
    last_keyframe = -p->i_keyint_max;
    badapt = c.bframes ? p->i_bframe_adaptive : 0;
    if (badapt || p->i_scenecut_threshold > 0 || c.mbtree || rc.vbv_lookahead) {
        if (x264gpu_slicetype_create(&st, p->i_width, p->i_height, 1, c.slots, c.bframes, p->analyse.i_me_method, p->analyse.i_subpel_refine, p->analyse.i_me_range,
                                     p->analyse.b_weighted_bipred, p->analyse.i_mv_range, c.mbtree || c.vbv ? 1 : 0) != X264GPU_OK) {
            xlog(p, X264_LOG_ERROR, "GPU lookahead setup failed: %s\n", x264gpu_last_error());
            return false;
        }
        param.i_bframe_bias = clampi(p->i_bframe_bias, -90, 100);
        (void)x264gpu_slicetype_set_bframe_bias(st, p->i_bframe_bias);          // --b-bias also scales the B costs of slicetype_frame_cost
    }
    aq_costs = st && !c.mbtree && c.aq_strength != 0.f && rc.by_cost();
    return true;
}

void SliceType::close() { if (st) x264gpu_slicetype_destroy(st); st = nullptr; }

bool SliceType::put(Frame &fr, const uint8_t *d_raw, int asked)
{
    if (st) {
        // the slice-type analysis decides keyframes and scene cuts itself: only what the caller forced stays forced
        fr.forced = asked;
        fr.scenecut = 0;
        const size_t slot = (size_t)fr.slot, offsets = (size_t)(c.mbw * c.mbh) * sizeof(float);
        bool ok = x264gpu_slicetype_put_frame(st, fr.slot, d_raw, nullptr) == X264GPU_OK;
        if (ok && c.weightp) { uint64_t stats[2]; ok = x264gpu_slicetype_pixel_stats(st, fr.slot, d_raw, stats, nullptr) == X264GPU_OK; }      // x264_adaptive_quant_frame: i_pixel_sum / i_pixel_ssd
        if (ok && c.mbtree) {
            // x264_adaptive_quant_frame: the AQ offsets weight the lookahead's costs and are what the tree starts from (f_qp_offset = f_qp_offset_aq)
            if (c.aq_strength == 0.f) ok = x264gpu_memset(c.q_aq[slot], 0, offsets, nullptr) == X264GPU_OK;
            ok = ok && x264gpu_slicetype_set_aq(st, fr.slot, c.aq_strength != 0.f ? c.q_aq[slot] : nullptr, nullptr) == X264GPU_OK &&
                 x264gpu_memcpy_d2d(c.q_tree[slot], c.q_aq[slot], offsets, nullptr) == X264GPU_OK;
        }
        if (ok && aq_costs) ok = x264gpu_slicetype_set_aq(st, fr.slot, c.q_aq[slot], nullptr) == X264GPU_OK;      // i_inv_qscale_factor for i_cost_est_aq
        if (!ok) return false;
    }
    bq.push_back(fr);
    return true;
}

void SliceType::cost_failed() { xlog(p, X264_LOG_ERROR, "lookahead frame cost failed: %s\n", x264gpu_last_error()); failed = true; }
static int forced_type(const SliceType::Frame &e) { return e.forced == 2 ? ST_IDR : e.forced == 1 ? ST_I : ST_AUTO; }
void SliceType::reset_types() { for (Frame &e : bq) e.type = forced_type(e); }

// x264_weights_analyse: guess scale and offset of each plane from the two pictures' statistics, cost the candidates around the guess — luma on the
// half-resolution planes (per 8x8 block min(mbcmp, intra cost)), the chroma planes at full resolution on the blocks' DC differences — keep a weight
// if it saves more than 0.2 %.  b_lookahead: luma alone, the guess alone, reference in place (called before a P cost is searched); else, for the P
// picture about to be coded: +- the distances of the sub-pel level around the guess, the reference motion-compensated by the lookahead's vectors,
// and the chroma planes once luma has a weight.
Dpb::LumaWeight SliceType::weights_analyse(Frame &fenc, const Frame &ref, int dist, bool b_lookahead)
{
    Dpb::LumaWeight none, w;
    if (dist >= 1 && dist <= 18) fenc.weighted_cost_delta[dist - 1] = 0;
    uint64_t sf[6], sr[6];
    const uint8_t *raw_f = c.q_raw[(size_t)fenc.slot], *raw_r = c.q_raw[(size_t)ref.slot];
    if (x264gpu_slicetype_pixel_stats(st, fenc.slot, raw_f, sf, nullptr) != X264GPU_OK ||
        x264gpu_slicetype_pixel_stats(st, ref.slot, raw_r, sr, nullptr) != X264GPU_OK) { failed = true; return none; }
    const int nplanes = b_lookahead ? 1 : 3;
    if (!b_lookahead && (x264gpu_slicetype_chroma_stats(st, fenc.slot, raw_f, sf + 2, nullptr) != X264GPU_OK ||
                         x264gpu_slicetype_chroma_stats(st, ref.slot, raw_r, sr + 2, nullptr) != X264GPU_OK)) { failed = true; return none; }
    const float epsilon = 1.f / 128.f;
    float guess_scale[3] = { 1, 1, 1 }, fenc_mean[3] = { 0, 0, 0 }, ref_mean[3] = { 0, 0, 0 };
    for (int plane = 0; plane < nplanes; plane++) {
        const int zero_bias = !sr[2 * plane + 1];
        const float fenc_var = (float)(sf[2 * plane + 1] + (uint64_t)zero_bias), ref_var = (float)(sr[2 * plane + 1] + (uint64_t)zero_bias);
        guess_scale[plane] = sqrtf(fenc_var / ref_var);
        const float npix = plane ? (float)(c.mbw * 8) * (float)(c.mbh * 8) : (float)(c.mbw * 16) * (float)(c.mbh * 16);
        fenc_mean[plane] = (float)(sf[2 * plane] + (uint64_t)zero_bias) / npix; ref_mean[plane] = (float)(sr[2 * plane] + (uint64_t)zero_bias) / npix;
    }
    int chroma_denom = 7;
    if (!b_lookahead)          // make sure both chroma scale factors fit
        while (chroma_denom > 0) {
            const float thresh = 127.f / (1 << chroma_denom);
            if (guess_scale[1] < thresh && guess_scale[2] < thresh) break;
            chroma_denom--;
        }
    static const uint8_t check_distance[12][2] = { { 0, 0 }, { 0, 0 }, { 0, 1 }, { 0, 1 }, { 0, 1 }, { 0, 1 }, { 0, 1 }, { 1, 1 }, { 1, 1 }, { 2, 1 }, { 2, 1 }, { 4, 2 } };
    const int sub = clampi(p->analyse.i_subpel_refine, 0, 11);
    const int scale_dist = b_lookahead ? 0 : check_distance[sub][0], offset_dist = b_lookahead ? 0 : check_distance[sub][1];
    bool planes_on[3] = { false, false, false };
    int p_scale[3] = { 1, 1, 1 }, p_denom[3] = { 0, 0, 0 }, p_off[3] = { 0, 0, 0 };
    // (the chroma planes are not checked in the lookahead, or if there was no luma weight)
    for (int plane = 0; plane < nplanes && !(plane && !planes_on[0]); plane++) {
        if (fabsf(ref_mean[plane] - fenc_mean[plane]) < 0.5f && fabsf(1.f - guess_scale[plane]) < epsilon) continue;      // early termination
        int mindenom, minscale, minoff = 0;
        if (plane) {
            mindenom = chroma_denom;
            minscale = clampi((int)roundf(guess_scale[plane] * (1 << chroma_denom)), 0, 255);
            if (minscale > 127) { planes_on[1] = planes_on[2] = false; break; }
        } else {
            // weight_get_h264( round( guess_scale * 128 ), 0 )
            mindenom = 7; minscale = (int)roundf(guess_scale[0] * 128);
            while (mindenom > 0 && minscale > 127) { mindenom--; minscale >>= 1; }
            if (minscale > 127) minscale = 127;
        }
        auto cost_of = [&](int on, int scale, int denom, int offset, int64_t &score) {
            if (!plane) return x264gpu_slicetype_weight_cost(st, fenc.slot, ref.slot, dist, on, scale, denom, offset, &score, nullptr) == X264GPU_OK;
            return x264gpu_slicetype_weight_cost_chroma(st, fenc.slot, raw_f, raw_r, dist, plane, on, scale, denom, offset, &score, nullptr) == X264GPU_OK;
        };
        int32_t dummy = 0;
        int64_t score = 0;
        if ((!plane && x264gpu_slicetype_frame_cost(st, fenc.slot, fenc.slot, fenc.slot, 0, 0, &dummy, nullptr) != X264GPU_OK) ||       // the picture's intra costs
            !cost_of(0, 1, 0, 0, score)) { failed = true; return none; }
        const unsigned origscore = (unsigned)score;
        unsigned minscore = origscore;
        if (!minscore) continue;
        const int start_scale = clampi(minscale - scale_dist, 0, 127), end_scale = clampi(minscale + scale_dist, 0, 127);
        bool found = false;
        for (int i_scale = start_scale; i_scale <= end_scale; i_scale++) {
            int cur_scale = i_scale;
            int cur_offset = (int)(fenc_mean[plane] - ref_mean[plane] * cur_scale / (1 << mindenom) + 0.5f * b_lookahead);
            if (cur_offset < -128 || cur_offset > 127) {
                cur_offset = clampi(cur_offset, -128, 127);
                float cs = (1 << mindenom) * (fenc_mean[plane] - cur_offset) / ref_mean[plane] + 0.5f;
                cur_scale = (int)(cs < 0 ? 0 : cs > 127 ? 127 : cs);
            }
            const int start_offset = clampi(cur_offset - offset_dist, -128, 127), end_offset = clampi(cur_offset + offset_dist, -128, 127);
            for (int i_off = start_offset; i_off <= end_offset; i_off++) {
                if (!cost_of(1, cur_scale, mindenom, i_off, score)) { failed = true; return none; }
                if ((unsigned)score < minscore) { minscore = (unsigned)score; minscale = cur_scale; minoff = i_off; found = true; }
                if (minoff == start_offset && i_off != start_offset) break;          // the previous offset was better: no more
            }
        }
        if (!plane) while (mindenom > 0 && !(minscale & 1)) { mindenom--; minscale >>= 1; }      // a smaller denominator if possible
        if (!found || (minscale == 1 << mindenom && minoff == 0) || (float)minscore / origscore > 0.998f) continue;
        planes_on[plane] = true; p_scale[plane] = minscale; p_denom[plane] = mindenom; p_off[plane] = minoff;
        if (weightp_fake && !plane && dist >= 1 && dist <= 18) fenc.weighted_cost_delta[dist - 1] = (float)minscore / origscore;
    }
    if (!planes_on[0]) return none;           // (x264 keeps chroma weights only beside a luma weight: they are not even analysed without one)
    w.on = 1; w.scale = p_scale[0]; w.denom = p_denom[0]; w.offset = p_off[0];
    if (planes_on[1] || planes_on[2]) {
        // optimise and unify the chroma denominator: a plane weighted alone leaves the other with the implicit scale 1 << denom, which 7 cannot carry
        int denom = planes_on[1] ? p_denom[1] : p_denom[2];
        const bool both = planes_on[1] && planes_on[2];
        while ((!both && denom == 7) || (denom > 0 && !(planes_on[1] && (p_scale[1] & 1)) && !(planes_on[2] && (p_scale[2] & 1)))) {
            denom--;
            for (int i = 1; i <= 2; i++) if (planes_on[i]) { p_scale[i] >>= 1; p_denom[i] = denom; }
        }
        w.cdenom = denom;
        for (int k = 0; k < 2; k++) if (planes_on[k + 1]) { w.con[k] = 1; w.cscale[k] = p_scale[k + 1]; w.coffset[k] = p_off[k + 1]; }
    }
    return w;
}

int SliceType::Window::frame_cost(int p0, int p1, int b)
{
    int32_t sc = 0;
    Dpb::LumaWeight w;
    // slicetype_frame_cost: a P cost that is searched for the first time runs on the reference weighted by the lookahead's analysis
    if ((s.c.weightp || s.weightp_fake) && p1 == b && b != p0 && !x264gpu_slicetype_lowres_mvs(s.st, fr(b).slot, 0, b - p0) &&
        x264gpu_slicetype_cost_est(s.st, fr(b).slot, b - p0, 0, 0) < 0)
        w = s.weights_analyse(fr(b), fr(p0), b - p0, true);
    if (x264gpu_slicetype_frame_cost_w(s.st, fr(p0).slot, fr(p1).slot, fr(b).slot, b - p0, p1 - b, w.on, w.scale, w.denom, w.offset, &sc, nullptr) != X264GPU_OK)
        s.cost_failed();
    return sc;
}
// scenecut_internal: P cost against I cost of frames[p1], the bias growing with the distance from the last keyframe
bool SliceType::Window::scenecut_internal(int p0, int p1)
{
    const x264_param_t &p = *s.p;
    frame_cost(p0, p1, p1);
    const int icost = x264gpu_slicetype_cost_est(s.st, fr(p1).slot, 0, 0, 0), pcost = x264gpu_slicetype_cost_est(s.st, fr(p1).slot, p1 - p0, 0, 0);
    const int gop = fr(p1).frame - s.last_keyframe;
    const float tmax = (float)(p.i_scenecut_threshold / 100.0);
    float tmin = (float)(tmax * 0.25), bias;
    if (p.i_keyint_min == p.i_keyint_max) tmin = tmax;
    if (gop <= p.i_keyint_min / 4) bias = tmin / 4;
    else if (gop <= p.i_keyint_min) bias = tmin * gop / p.i_keyint_min;
    else bias = tmin + (tmax - tmin) * (gop - p.i_keyint_min) / (p.i_keyint_max - p.i_keyint_min);
    return pcost >= (1.0 - bias) * icost;
}
// scenecut: with B pictures a short flash between two scenes must not become a keyframe (x264 looks one picture past p1 under --b-adapt 1)
bool SliceType::Window::scenecut(int p0, int p1, bool real, int num_frames, int i_max_search)
{
    if (real && s.c.bframes) {
        const int origmaxp1 = p0 + 1 + (s.badapt == 2 ? s.c.bframes : 1), maxp1 = origmaxp1 < num_frames ? origmaxp1 : num_frames;      // the trellis may put bframes pictures between p0 and p1
        for (int curp1 = p1; curp1 <= maxp1; curp1++)
            if (!scenecut_internal(p0, curp1))
                for (int i = curp1; i > p0; i--) fr(i).b_scenecut = 0;          // nothing between p0 and curp1 can be a real scene cut
        for (int curp0 = p0; curp0 <= maxp1; curp0++)
            if (origmaxp1 > i_max_search || (curp0 < maxp1 && scenecut_internal(curp0, maxp1)))
                fr(curp0).b_scenecut = 0;                                     // the p0 of a scene cut cannot be the p1 of one
    }
    if (!fr(p1).b_scenecut) return false;
    return scenecut_internal(p0, p1);
}
// x264's macroblock_tree over frames[0 .. num_frames] with the types decided so far (tests/mbtree_walk.py is the same walk): every picture hands
// the cost its references explain back to them, last picture first; the next picture to be coded (and the B-reference of its run) get their
// quantiser offsets.  b_intra: the pass x264 runs for a keyframe after it was decided (frames[0] = that keyframe).
void SliceType::Window::macroblock_tree(int num_frames, bool b_intra)
{
    const int idx = b_intra ? 0 : 1;
    auto slot = [&](int i) { return fr(i).slot; };
    auto prop = [&](int p0, int p1, int b, int referenced) {
        if (x264gpu_slicetype_propagate(s.st, slot(p0), slot(p1), slot(b), b - p0, p1 - b, referenced, nullptr) != X264GPU_OK) {
            xlog(s.p, X264_LOG_ERROR, "macroblock-tree failed: %s\n", x264gpu_last_error());
            s.failed = true;
        }
    };
    auto clear = [&](int i) { if (x264gpu_slicetype_clear_propagate(s.st, slot(i), nullptr) != X264GPU_OK) s.failed = true; };
    auto finish = [&](int i, int ref0_distance) {
        frame_cost(i, i, i);          // (the intra costs the analysis left with the picture; a no-op when they exist)
        // macroblock_tree_finish: a fade the (fake) weight analysis explained is not held against the picture
        float weightdelta = 0.0;
        if (ref0_distance >= 1 && ref0_distance <= 18 && fr(i).weighted_cost_delta[ref0_distance - 1] > 0) weightdelta = (float)(1.0 - fr(i).weighted_cost_delta[ref0_distance - 1]);
        if (x264gpu_slicetype_finish(s.st, slot(i), s.c.tree_strength, weightdelta, s.c.q_tree[(size_t)slot(i)], nullptr) != X264GPU_OK) s.failed = true;
    };
    if (b_intra) frame_cost(0, 0, 0);
    int i = num_frames;
    while (i > 0 && isb(i)) i--;
    int last_nonb = i, bframes = 0;
    if (last_nonb < idx) return;
    clear(last_nonb);
    while (i-- > idx) {
        int cur_nonb = i;
        while (isb(cur_nonb) && cur_nonb > 0) cur_nonb--;
        if (cur_nonb < idx) break;
        // (distances beyond bframes + 1 cannot occur: the analysis never leaves longer runs)
        frame_cost(cur_nonb, last_nonb, last_nonb);
        clear(cur_nonb);
        bframes = last_nonb - cur_nonb - 1;
        if (s.c.bpyramid && bframes > 1) {
            const int middle = (bframes + 1) / 2 + cur_nonb;
            frame_cost(cur_nonb, last_nonb, middle);
            clear(middle);
            while (i > cur_nonb) {
                const int p0 = i > middle ? middle : cur_nonb, p1 = i < middle ? middle : last_nonb;
                if (i != middle) { frame_cost(p0, p1, i); prop(p0, p1, i, 0); }
                i--;
            }
            prop(cur_nonb, last_nonb, middle, 1);
        } else
            while (i > cur_nonb) { frame_cost(cur_nonb, last_nonb, i); prop(cur_nonb, last_nonb, i, 0); i--; }
        prop(cur_nonb, last_nonb, last_nonb, 1);
        last_nonb = cur_nonb;
        if (s.failed) return;
    }
    finish(last_nonb, last_nonb);
    if (s.c.bpyramid && bframes > 1) finish(last_nonb + (bframes + 1) / 2, 0);
}

// x264 slicetype_path_cost: the cost of coding frames[1 ..] with the types in `path` ('P' / 'B' / 'I' per picture) — each non-B picture against the one
// before it, the B pictures between them against both (through the middle one under b-pyramid); stops early beyond `threshold`
uint64_t SliceType::Window::path_cost(const char *path0, uint64_t threshold)
{
    uint64_t cost = 0;
    int loc = 1, cur_nonb = 0;
    const char *path = path0 - 1;          // the first path element is the second frame
    while (path[loc]) {
        int next_nonb = loc;
        while (path[next_nonb] == 'B') next_nonb++;
        cost += path[next_nonb] == 'P' ? frame_cost(cur_nonb, next_nonb, next_nonb) : frame_cost(next_nonb, next_nonb, next_nonb);
        if (cost > threshold || s.failed) break;
        if (s.c.bpyramid && next_nonb - cur_nonb > 2) {
            const int middle = cur_nonb + (next_nonb - cur_nonb) / 2;
            cost += frame_cost(cur_nonb, next_nonb, middle);
            for (int next_b = loc; next_b < middle && cost < threshold; next_b++) cost += frame_cost(cur_nonb, middle, next_b);
            for (int next_b = middle + 1; next_b < next_nonb && cost < threshold; next_b++) cost += frame_cost(middle, next_nonb, next_b);
        } else
            for (int next_b = loc; next_b < next_nonb && cost < threshold; next_b++) cost += frame_cost(cur_nonb, next_nonb, next_b);
        loc = next_nonb + 1;
        cur_nonb = next_nonb;
    }
    return cost;
}

// x264 slicetype_path (--b-adapt 2): the best way to code the first `length` pictures ends in 0 .. bframes B pictures and a P picture behind the
// best way to code the pictures in front of them (Viterbi over the lengths; best_paths is indexed by length modulo 17)
void SliceType::Window::path(int length, char (*best_paths)[ST_PATH_MAX + 1])
{
    char paths[2][ST_PATH_MAX + 1];
    const int num_paths = s.c.bframes + 1 < length ? s.c.bframes + 1 : length;
    uint64_t best_cost = ~0ull >> 1;
    int best_possible = 0, idx = 0;
    memset(paths, 0, sizeof(paths));
    for (int path = 0; path < num_paths; path++) {
        const int len = length - (path + 1);
        memcpy(paths[idx], best_paths[len % 17], (size_t)len);
        memset(paths[idx] + len, 'B', (size_t)path);
        paths[idx][len + path] = 'P'; paths[idx][len + path + 1] = 0;
        int possible = 1;
        for (int i = 1; i <= length; i++) {
            const int t = fr(i).type;
            if (t == ST_AUTO) continue;
            if (is_b(t)) possible = possible && (i < len || i == length || paths[idx][i - 1] == 'B');
            else {
                possible = possible && (i < len || paths[idx][i - 1] != 'B');
                paths[idx][i - 1] = t == ST_I || t == ST_IDR ? 'I' : 'P';
            }
        }
        if (possible || !best_possible) {
            if (possible && !best_possible) best_cost = ~0ull >> 1;
            const uint64_t cost = path_cost(paths[idx], best_cost);
            if (cost < best_cost) { best_cost = cost; best_possible = possible; idx ^= 1; }
        }
    }
    memcpy(best_paths[length % 17], paths[idx ^ 1], (size_t)length);
    best_paths[length % 17][length] = 0;
}

// x264's vbv_lookahead: the pictures of the window in coding order (each non-B picture, then the B pictures in front of it) with the types the analysis gave them
// and their frame costs (vbv_frame_cost: the AQ-weighted ones in AQ sessions), left with the picture that is coded next — the first non-B picture of the window,
// or (keyframe) frames[0] itself, a keyframe that has just been decided.  The window's last picture is not part of the plan, as in x264
void SliceType::Window::vbv_lookahead(int num_frames, bool keyframe)
{
    auto vbv_frame_cost = [&](int p0, int p1, int b) {
        int32_t cost = frame_cost(p0, p1, b);
        if (!s.failed && s.c.aq_strength != 0.f && (s.c.mbtree || s.aq_costs) &&
            x264gpu_slicetype_cost_aq(s.st, fr(b).slot, b - p0, p1 - b, &cost, nullptr) != X264GPU_OK)
            s.cost_failed();
        return cost;
    };
    int last_nonb = 0, cur_nonb = 1, idx = 0;
    while (cur_nonb < num_frames && isb(cur_nonb)) cur_nonb++;
    const int next_nonb = keyframe ? last_nonb : cur_nonb;
    RateControl::Planned &pl = fr(next_nonb).planned;
    while (cur_nonb < num_frames && idx < RateControl::PLAN_MAX && !s.failed) {
        if (next_nonb != cur_nonb) {          // the P / I picture (its cost as the type it was given; not next_nonb's own)
            const int t = fr(cur_nonb).type;
            const bool is_i = t == ST_I || t == ST_IDR;
            pl.satd[idx] = vbv_frame_cost(is_i ? cur_nonb : last_nonb, cur_nonb, cur_nonb);
            pl.type[idx] = t == ST_IDR ? PIC_IDR : t == ST_I ? PIC_I : PIC_P;
            idx++;
        }
        for (int i = last_nonb + 1; i < cur_nonb && idx < RateControl::PLAN_MAX; i++, idx++) {          // the B pictures, coded behind it
            pl.satd[idx] = vbv_frame_cost(last_nonb, cur_nonb, i);
            pl.type[idx] = PIC_B;
        }
        last_nonb = cur_nonb;
        cur_nonb++;
        while (cur_nonb <= num_frames && isb(cur_nonb)) cur_nonb++;
    }
    pl.type[idx] = RateControl::PLAN_END;
}

void SliceType::Window::analyse(int framecnt, bool keyframe)
{
    const x264_param_t &p = *s.p;
    auto type = [&](int i) -> int & { return fr(i).type; };
    auto forced = [&](int i) { return forced_type(fr(i)); };
    auto auto_or_i = [](int t) { return t == ST_AUTO || t == ST_I || t == ST_IDR; };
    const int i_max_search = framecnt;
    if (!framecnt) return;
    const int keyint_limit = p.i_keyint_max - f[0]->frame + s.last_keyframe - 1;
    int num_frames = framecnt < keyint_limit ? framecnt : keyint_limit;
    const int orig_num_frames = num_frames;
    if (p.analyse.b_psy && s.c.mbtree) num_frames = framecnt;           // psy-wise the pictures before a keyframe must not lose their share of the tree
    else if (num_frames <= 0) { type(1) = ST_I; return; }
    // a picture whose type the caller forced ends the window in front of it (x264 warns and overrides; here the analysis stops short)
    for (int j = 2; j <= num_frames; j++) if (forced(j) != ST_AUTO) { num_frames = j - 1; break; }
    if (!keyframe && auto_or_i(type(1)) && p.i_scenecut_threshold && scenecut(0, 1, true, orig_num_frames, i_max_search)) {
        if (type(1) == ST_AUTO) type(1) = ST_I;
        return;
    }
    int num_bframes = 0, reset_start, num_analysed = num_frames;
    if (s.c.bframes) {
        if (s.badapt == 2) {
            if (num_frames > ST_PATH_MAX) num_frames = ST_PATH_MAX;
            if (num_frames > 1) {
                static thread_local char best_paths[17][ST_PATH_MAX + 1];
                memset(best_paths, 0, sizeof(best_paths));
                best_paths[1][0] = 'P';
                const int best_path_index = num_frames % 17;
                for (int j = 2; j <= num_frames && !s.failed; j++) path(j, best_paths);
                if (s.failed) return;
                for (int j = 1; j < num_frames; j++) {
                    if (best_paths[best_path_index][j - 1] != 'B') { if (type(j) == ST_AUTO || isb(j)) type(j) = ST_P; }
                    else if (type(j) == ST_AUTO) type(j) = ST_B;
                }
            }
            if (type(num_frames) == ST_AUTO || isb(num_frames)) type(num_frames) = ST_P;
            while (num_bframes < num_frames && type(num_bframes + 1) == ST_B) num_bframes++;
        } else if (s.badapt == 1) {
            // X264_B_ADAPT_FAST as the x264 generation this host restates has it (the one whose trellis loader and scene-cut loop know forced types): picture j becomes
            // a B picture when the path "..BP" from the last non-B picture costs less than "..PP" (slicetype_path_cost on both), runs no longer than --bframes.
            // (Older x264 compared pairwise frame costs against thresholds — INTER_THRESH / P_SENS_BIAS; which of the two the driver's core 157 carries cannot be
            // checked here: DESIGN.md §0.)
            int last_nonb = 0, num_bf = s.c.bframes;
            char path[ST_PATH_MAX + 4];
            for (int j = 1; j < num_frames && !s.failed; j++) {
                if (j - 1 > 0 && isb(j - 1)) num_bf--;
                else { last_nonb = j - 1; num_bf = s.c.bframes; }
                if (!num_bf) { if (type(j) == ST_AUTO || isb(j)) type(j) = ST_P; continue; }
                if (type(j) != ST_AUTO) continue;
                if (isb(j + 1)) { type(j) = ST_P; continue; }
                const int bfr = j - last_nonb - 1;
                Window sub(s, rc);
                sub.f.assign(f.begin() + last_nonb, f.end());
                memset(path, 'B', (size_t)bfr);
                strcpy(path + bfr, "PP");
                const uint64_t cost_p = sub.path_cost(path, ~0ull >> 1);
                strcpy(path + bfr, "BP");
                const uint64_t cost_b = sub.path_cost(path, cost_p);
                type(j) = cost_b < cost_p ? ST_B : ST_P;
            }
            if (s.failed) return;
            if (type(num_frames) == ST_AUTO || isb(num_frames)) type(num_frames) = ST_P;
            while (num_bframes < num_frames && type(num_bframes + 1) == ST_B) num_bframes++;
        } else {
            num_bframes = num_frames - 1 < s.c.bframes ? num_frames - 1 : s.c.bframes;
            for (int j = 1; j < num_frames; j++) type(j) = (j % (num_bframes + 1)) ? ST_B : ST_P;
            type(num_frames) = ST_P;
        }
        // scene cut inside the first mini-GOP: the picture in front of it closes the run
        for (int j = 1; j < num_bframes + 1; j++)
            if (forced(j) == ST_AUTO && auto_or_i(forced(j + 1)) && p.i_scenecut_threshold && scenecut(j, j + 1, false, orig_num_frames, i_max_search)) {
                type(j) = ST_P;
                num_analysed = j;
                break;
            }
        reset_start = keyframe ? 1 : num_bframes + 2 < num_analysed + 1 ? num_bframes + 2 : num_analysed + 1;
    } else {
        for (int j = 1; j <= num_frames; j++) if (auto_or_i(forced(j))) type(j) = ST_P;
        reset_start = keyframe ? 1 : 2;
    }
    // the macroblock-tree over the window, no farther than a keyframe interval
    if (s.c.mbtree) macroblock_tree(num_frames < p.i_keyint_max ? num_frames : p.i_keyint_max, keyframe);
    if (s.failed) return;
    // enforce the keyframe limit
    {
        int last_keyframe = s.last_keyframe, last_possible = 0;
        for (int j = 1; j <= num_frames; j++) {
            int kd = fr(j).frame - last_keyframe;
            if (auto_or_i(forced(j))) last_possible = j;
            if (kd >= p.i_keyint_max) {
                if (last_possible != 0 && last_possible != j) { j = last_possible; kd = fr(j).frame - last_keyframe; }
                last_possible = 0;
                if (type(j) != ST_IDR) type(j) = ST_IDR;
            }
            if (type(j) == ST_I && kd >= p.i_keyint_min) type(j) = ST_IDR;
            if (type(j) == ST_IDR) { last_keyframe = fr(j).frame; if (j > 1 && isb(j - 1)) type(j - 1) = ST_P; }
        }
    }
    if (rc.vbv_lookahead) vbv_lookahead(num_frames, keyframe);
    if (s.failed) return;
    // the pictures behind the first mini-GOP are decided again when their turn comes
    for (int j = reset_start; j <= framecnt; j++) type(j) = forced(j);
}

// x264_slicetype_decide: types the first mini-GOP of the queue -> index of the picture that closes it
int SliceType::decide_types(const RateControl &rc)
{
    const int n = (int)bq.size();
    reset_types();
    if (rc.pass2) {
        // x264_ratecontrol_slice_type: the second pass codes every picture as the type the first pass gave it (the B-reference of a run is placed by
        // the same rule in both passes)
        for (auto &e : bq) {
            const RateControl::Pass2Entry *pe = rc.plan(e.frame);
            if (!pe) continue;
            const char t = pe->type;
            e.type = t == 'I' ? ST_IDR : t == 'i' ? ST_I : t == 'P' ? ST_P : ST_B;
        }
    } else
    if (have_last_nonb && ((c.bframes && badapt) || p->i_scenecut_threshold || c.mbtree || rc.vbv_lookahead)) {
        Window F(*this, rc);
        const int framecnt = n < c.wait + 1 ? n : c.wait + 1;          // what the lookahead holds for sure (deterministic mode), except at the end
        for (int i = 0; i < framecnt; i++) F.f.push_back(&bq[(size_t)i]);
        F.analyse(framecnt);
        if (failed) return 0;
    }
    int bfr;
    for (bfr = 0;; bfr++) {
        Frame &frm = bq[(size_t)bfr];
        if (frm.frame - last_keyframe >= p->i_keyint_max) frm.type = ST_IDR;              // limit the GOP size
        if (frm.type == ST_I && frm.frame - last_keyframe >= p->i_keyint_min) frm.type = ST_IDR;
        if (frm.type == ST_IDR) {                                                          // close the GOP
            last_keyframe = frm.frame;
            // x264 keeps i_type on the frame; here the queue's types are re-derived from `forced` on every call, so the decision is pinned
            // there: the IDR stays an IDR when it is reached after the run in front of it (which closes as P) has been coded
            if (bfr > 0) { frm.forced = 2; bfr--; bq[(size_t)bfr].type = ST_P; }
        }
        if (bfr == c.bframes || bfr + 1 >= n) { if (frm.type == ST_AUTO || is_b(frm.type)) frm.type = ST_P; }
        if (frm.type == ST_AUTO) frm.type = ST_B;
        else if (!is_b(frm.type)) break;
    }
    return bfr;
}

// the mini-GOP bq[j] closes leaves the display-order queue in coding order: the closing picture, the B-reference of the run, the other B pictures
void SliceType::close_minigop(int j, int closing)
{
    coding.push_back({ bq[(size_t)j], closing });
    const int bref = c.bpyramid && j > 1 ? (j - 1) / 2 : -1;
    if (bref >= 0) coding.push_back({ bq[(size_t)bref], PIC_BREF });
    for (int i = 0; i < j; i++) if (i != bref) coding.push_back({ bq[(size_t)i], PIC_B });
    bq.erase(bq.begin(), bq.begin() + j + 1);
}

bool SliceType::decide(bool flushing, const RateControl &rc)
{
    if (!coding.empty() || bq.empty()) return !coding.empty();
    const int n = (int)bq.size();
    if (!flushing && n <= (st ? c.wait : c.bframes)) return false;          // the lookahead x264 keeps in front of the slice-type decision
    if (st) {
        const int j = decide_types(rc);
        if (failed) return false;
        Frame &cl = bq[(size_t)j];
        const int closing = cl.type == ST_IDR ? PIC_IDR : cl.type == ST_I ? PIC_I : PIC_P;
        const bool isp = closing == PIC_P && have_last_nonb;
        if (c.weightp && isp) {
            // x264_slicetype_decide: "analyse for weighted P frames" — the picture about to be coded against the last non-B picture
            cl.w = weights_analyse(cl, last_nonb, j + 1, false);
            if (failed) return false;
        }
        if (rc.by_cost()) {
            // x264_rc_analyse_slice: the closing picture's complexity is its frame cost as the type it was given — the I cost, or the P cost
            // against the last non-B picture (distance = run length + 1), from the lookahead that decided the types
            int32_t ic = 0, pc = 0;
            bool ok = x264gpu_slicetype_frame_cost(st, cl.slot, cl.slot, cl.slot, 0, 0, &ic, nullptr) == X264GPU_OK;
            if (ok && isp) ok = x264gpu_slicetype_frame_cost(st, last_nonb.slot, cl.slot, cl.slot, j + 1, 0, &pc, nullptr) == X264GPU_OK;
            else pc = ic;
            if (ok && aq_costs) {
                // x264_rc_analyse_slice: "in AQ, use the weighted score instead" (without macroblock-tree; with it the rate factor does not read the cost)
                ok = x264gpu_slicetype_cost_aq(st, cl.slot, 0, 0, &ic, nullptr) == X264GPU_OK && (!isp || x264gpu_slicetype_cost_aq(st, cl.slot, j + 1, 0, &pc, nullptr) == X264GPU_OK);
                if (!isp) pc = ic;
            }
            if (!ok) { cost_failed(); return false; }
            cl.costs[0] = ic; cl.costs[1] = pc;
        }
        last_nonb = cl; have_last_nonb = true;
        close_minigop(j, closing);
        if ((c.mbtree || rc.vbv_lookahead) && (closing == PIC_IDR || closing == PIC_I)) {
            // x264 lookahead_slicetype_decide: "for MB-tree and VBV lookahead, we have to perform propagation analysis on I-frames too" — the analysis again
            // with the keyframe as frames[0]; it decides nothing, its tree reaches the keyframe itself, its plan is the keyframe's
            Window F(*this, rc);
            const int n2 = (int)bq.size(), room = c.wait - j, framecnt = n2 < room ? n2 : room > 0 ? room : 0;          // (what is left of the window behind the mini-GOP)
            reset_types();
            for (int i = 0; i < framecnt; i++) F.f.push_back(&bq[(size_t)i]);
            if (framecnt > 0) F.analyse(framecnt, true);
            else if (c.mbtree) F.macroblock_tree(0, true);
            if (failed) return false;
            coding.front().e.planned = last_nonb.planned;          // (the closing picture was queued before its plan was made)
        }
        return true;
    }
    // the fixed picture structure: a forced I / IDR picture closes the run in front of it, otherwise the run is `bframes` long, or what is left when the input ends
    int j = -1;                                       // index of the closing picture
    if (bq[0].forced) j = 0;
    else {
        for (int i = 0; i < n && i <= c.bframes; i++) {
            if (bq[(size_t)i].forced == 2) { j = i > 0 ? i - 1 : 0; break; }        // IDR next: the picture before it closes the run as P
            if (bq[(size_t)i].forced == 1) { j = i; break; }                        // I picture: B pictures in front of it may predict from it
            if (i == c.bframes) { j = i; break; }
        }
        if (j < 0) { if (!flushing) return false; j = n - 1; }                      // end of input: the last picture closes the run
    }
    close_minigop(j, bq[(size_t)j].forced == 2 ? PIC_IDR : bq[(size_t)j].forced == 1 ? PIC_I : PIC_P);
    return true;
}

}  // namespace x264host

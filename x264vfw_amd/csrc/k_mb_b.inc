// k_mb_b.inc — B slices: the analysis and the sequence of RD candidates of one macroblock (included inside k_mb_slice's pass loop, BS
// instantiations only; restates oracle/analyse.c macroblock_b = [x264-upstream] encoder/analyse.c x264_macroblock_analyse, SLICE_TYPE_B branch
// with i_mbrd 1).  Runs at the top of a pass while the macroblock is undecided (rd_run && !commit): steps through rd_ph until a candidate
// is set up for the encode stage below (e_type / e_part / e_t8 / ecfg / euse) or the final pass is due (commit).
//
//   ph 0      direct prediction, B_SKIP on its distortion alone, SATD costs of direct, both lists' 16x16 searches, the bi-predictive 16x16
//   ph 1..4   early x264_mb_analyse_b_rd (direct within 33/32 of the best 16x16): direct, L0, L1, BI         ph 5  B_SKIP if it beats them all
//   ph 6      8x8 (mixed references or the 16x16 references), 16x8 / 8x16 in the order of their estimates
//   ph 7..13  x264_mb_analyse_b_rd: direct, L0, L1, BI, 8x8, 16x8, 8x16 (those within the threshold, not yet costed)
//   ph 14     decision among the inter types, intra analysis, the other transform size of the winner      ph 15..17  I16x16, I4x4, I8x8
//   ph 18     final decision, x264_refine_bidir, the real pass
for (;; rd_ph++) {
    bool go = false;
    RELANE();
    STATE_UNIFORM();
    auto use16_cfg = [&](int use) __attribute__((always_inline)) {          // the 16x16 candidate of list 0 / list 1 / both
        const int s0 = use == 2 ? 32 : 0, s1 = use == 2 ? 48 : 16;
        ecfg.r0 = use == 1 ? -1 : rl(S.ref, s0); ecfg.x0 = use == 1 ? 0 : rl(S.mvx, s0); ecfg.y0 = use == 1 ? 0 : rl(S.mvy, s0);
        ecfg.r1 = use == 0 ? -1 : rl(S.ref, s1); ecfg.x1 = use == 0 ? 0 : rl(S.mvx, s1); ecfg.y1 = use == 0 ? 0 : rl(S.mvy, s1);
        euse = (unsigned)use * 0x55u;
        e_type = X264GPU_MB_B_INTER; e_part = D_16x16;
    };
    // the candidate of a partitioned shape from the per-block / per-half decisions: this lane's block b8 = lane >> 4
    auto shape_cfg = [&](int part) __attribute__((always_inline)) {
        const int b8 = lane >> 4;
        const int k0 = part == D_8x8 ? b8 : part == D_16x8 ? b8 >> 1 : b8 & 1;                                   // block / half index
        const int base = part == D_8x8 ? ME_8 : part == D_16x8 ? ME_16x8 : ME_8x16;
        // (packed first: a chain of selects over variables captured by reference becomes a select of POINTERS into the closure, which pins the
        // closure and everything it captures — the whole search state — in scratch memory)
        const unsigned u8 = (unsigned)sub8_0 | ((unsigned)sub8_1 << 2) | ((unsigned)sub8_2 << 4) | ((unsigned)sub8_3 << 6);
        const unsigned uh = part == D_16x8 ? (unsigned)p16x8_0 | ((unsigned)p16x8_1 << 2) : (unsigned)p8x16_0 | ((unsigned)p8x16_1 << 2);
        const int use = (int)(((part == D_8x8 ? u8 : uh) >> (2 * k0)) & 3u);
        const int sl = base + k0;
        const int r0 = __shfl(S.ref, sl), x0 = __shfl(S.mvx, sl), y0 = __shfl(S.mvy, sl), r1 = __shfl(S.ref, sl + 16), x1 = __shfl(S.mvx, sl + 16), y1 = __shfl(S.mvy, sl + 16);
        ecfg.r0 = use == 3 ? dcfg.r0 : use == 1 ? -1 : r0; ecfg.x0 = use == 3 ? dcfg.x0 : use == 1 ? 0 : x0; ecfg.y0 = use == 3 ? dcfg.y0 : use == 1 ? 0 : y0;
        ecfg.r1 = use == 3 ? dcfg.r1 : use == 0 ? -1 : r1; ecfg.x1 = use == 3 ? dcfg.x1 : use == 0 ? 0 : x1; ecfg.y1 = use == 3 ? dcfg.y1 : use == 0 ? 0 : y1;
        if (part == D_8x8) euse = (unsigned)sub8_0 | ((unsigned)sub8_1 << 2) | ((unsigned)sub8_2 << 4) | ((unsigned)sub8_3 << 6);
        else if (part == D_16x8) euse = (unsigned)p16x8_0 * 5u | (unsigned)p16x8_1 * 0x50u;
        else euse = (unsigned)p8x16_0 * 0x11u | (unsigned)p8x16_1 * 0x44u;
        e_type = part == D_8x8 ? X264GPU_MB_B_8x8 : X264GPU_MB_B_INTER; e_part = part;
    };
    auto cmp4 = [&](uint32_t e, uint32_t p) __attribute__((always_inline)) { return c.satd ? satd4_half(e, p, lane) : sad4(e, p); };      // h->pixf.mbcmp: SATD from subme 2 up
    auto direct_cand = [&](int type) __attribute__((always_inline)) { ecfg = dcfg; euse = 0xffu; e_type = type; e_part = D_16x16; };
    auto winner_cfg = [&]() __attribute__((always_inline)) {
        if (b_type == X264GPU_MB_B_SKIP || b_type == X264GPU_MB_B_DIRECT) direct_cand(b_type);
        else if (b_part == D_16x16) use16_cfg(b_use16);
        else shape_cfg(b_part);
    };
    // SATD (+ chroma SATD under chroma-ME) of the bi-prediction of the blocks in mask8 from the result slots sl0 (list 0) / sl0 + 16 (list 1)
    auto bi_satd = [&](const BCfg &g, unsigned mask8, int &chroma_part) __attribute__((always_inline)) {
        uint32_t pred, cpred;
        b_predict(k, c, g, biwv, pred, cpred);
        const int h = (mask8 >> (lane >> 4)) & 1 ? cmp4(cz, pred) : 0;
        chroma_part = 0;
        if (c.chroma_me) {
            const int hc = lane < 32 && ((mask8 >> ((lane >> 2) & 3)) & 1) ? cmp4(b_cenc, cpred) : 0;
            chroma_part = wave_sum(hc);
        }
        return wave_sum(h);
    };
    auto refcost_l = [&](int l, int r) __attribute__((always_inline)) { return ref_bits(l ? k.nref1 : k.nref, r) * c.lambda; };
    // one block search of list l in reference r (x264_me_search_ref); the predictor comes from that list's motion cache
    auto search_b = [&](int l, int r, int part_kind, int bx8, int by8, int w8, int h8, int n_mvc, bool use_thresh, int &thr, int &mvx, int &mvy, int &cost, int &cost_mv, int &mvpx, int &mvpy) __attribute__((always_inline)) {
        MeJob jb;
        jb.search = true; jb.use_thresh = use_thresh; jb.n_mvc = n_mvc;
        jb.W = 8 * w8; jb.H = 8 * h8; jb.ox = 8 * bx8; jb.oy = 8 * by8; jb.ref = l ? k.nref + r : r;
        mb_predict_mv(S, part_kind, bx8, by8, w8, r, jb.mvpx, jb.mvpy, 16 * l);
        jb.hp_it = c.subme >= 2 ? (c.subme < 6 ? 1 : c.subme < 8 ? 2 : 4) : 0;          // subpel_iterations[subme][2..3]
        jb.qp_it = c.subme < 4 ? 0 : c.subme == 4 ? 1 : c.subme < 8 ? 2 : 10;
        mvpx = jb.mvpx; mvpy = jb.mvpy;
        lds_sync();
        mvx = 0; mvy = 0; cost = 0; cost_mv = 0;
        me_search<M, ME, false>(k, L, c, jb, mvx, mvy, cost, cost_mv, thr, S, wt, pf);
        lds_sync();
    };
    if (rd_ph == 0) {
        // ---- direct prediction in the slice's mode (x264_mb_predict_mv_direct16x16), motion-compensated.  --direct auto: the OTHER mode first, each
        //      probed for a skip and counted (h->stat.frame.i_direct_score: "prefer whichever mode allows more Skip macroblocks") ----
        const bool temporal_mode = k.direct_flags && k.direct_flags[s];
        uint32_t dpred = 0, dcpred = 0;
        bool probed = false;
        for (int pass = k.direct_auto ? 0 : 1; pass < 2; pass++) {
            const bool tmp = pass ? temporal_mode : !temporal_mode;
            d_avail = true;
            if (tmp) {
                // temporal (mb_predict_mv_direct16x16_temporal; 8.4.1.2.3): this lane's 8x8 block of the co-located macroblock in list 1's first picture — its
                // list-0 reference mapped into this picture's list 0, its vector scaled by the POC distances; no direct prediction when a block has none
                const bool icol = intra_t(uni((int)k.coltype[(size_t)s * k.nmb + mbi]));
                const size_t ci = ((size_t)s * k.nmb + mbi) * 4 + (lane >> 4);
                const int rc = icol ? -1 : (int)k.colref0[ci];
                int i_ref = -1, dsf = 256;
#pragma unroll
                for (int q = 0; q < 8; q++) if (rc == q) i_ref = k.map_col[q];
#pragma unroll
                for (int q = 0; q < 8; q++) if (i_ref == q) dsf = k.dist_scale[q];
                d_avail = icol || !__any(i_ref < 0);
                const uint32_t cm = icol ? 0u : ((const uint32_t *)k.colmv)[ci];
                const int cx = (int)(int16_t)(cm & 0xffff), cy = (int)(int16_t)(cm >> 16);
                const int l0x = (dsf * cx + 128) >> 8, l0y = (dsf * cy + 128) >> 8;
                dcfg.r0 = icol ? 0 : i_ref; dcfg.x0 = icol ? 0 : (int)(int16_t)l0x; dcfg.y0 = icol ? 0 : (int)(int16_t)l0y;
                dcfg.r1 = 0; dcfg.x1 = icol ? 0 : (int)(int16_t)(l0x - cx); dcfg.y1 = icol ? 0 : (int)(int16_t)(l0y - cy);
            } else {
        // ---- spatial direct prediction (x264_mb_predict_mv_direct16x16; 8.4.1.2.2) ----
        int dref[2], dmx[2], dmy[2];
#pragma unroll
        for (int l = 0; l < 2; l++) {
            const int go = 16 * l;
            const int ra = rl(S.cref, 4 + go), rb = rl(S.cref, 1 + go);
            const int ic = rl(S.cref, 3 + go) == -2 ? go : 3 + go;
            const int rc = rl(S.cref, ic);
            unsigned rm = (unsigned)ra < (unsigned)rb ? (unsigned)ra : (unsigned)rb;
            if ((unsigned)rc < rm) rm = (unsigned)rc;
            int ir = (int)rm, mx = 0, my = 0;
            if (ir < 0) ir = -1;
            else {
                const int ax = rl(S.cmvx, 4 + go), ay = rl(S.cmvy, 4 + go), bx = rl(S.cmvx, 1 + go), by = rl(S.cmvy, 1 + go), cx = rl(S.cmvx, ic), cy = rl(S.cmvy, ic);
                const int cnt = (ra == ir) + (rb == ir) + (rc == ir);
                if (cnt > 1) { mx = median3(ax, bx, cx); my = median3(ay, by, cy); }
                else if (ra == ir) { mx = ax; my = ay; } else if (rb == ir) { mx = bx; my = by; } else { mx = cx; my = cy; }
            }
            dref[l] = uni(ir); dmx[l] = uni(mx); dmy[l] = uni(my);
        }
        if (dref[0] < 0 && dref[1] < 0) { dref[0] = dref[1] = 0; }
        // colZeroFlag of the four 8x8 blocks (direct_8x8_inference): the co-located block of list 1's first picture points into ITS reference 0, within +-1
        unsigned czm = 0;
        {
            int cr = -1; uint32_t cm = 0;
            if (lane < 4) { cr = k.colref[((size_t)s * k.nmb + mbi) * 4 + lane]; cm = ((const uint32_t *)k.colmv)[((size_t)s * k.nmb + mbi) * 4 + lane]; }
            const int cx = (int)(int16_t)(cm & 0xffff), cy = (int)(int16_t)(cm >> 16);
            czm = (unsigned)(__ballot(lane < 4 && cr == 0 && cx >= -1 && cx <= 1 && cy >= -1 && cy <= 1) & 15);
        }
        const bool apply = (dmx[0] | dmy[0] | dmx[1] | dmy[1]) != 0 && !(dref[0] && dref[1]);
        {
            const bool z = apply && ((czm >> (lane >> 4)) & 1);
            dcfg.r0 = dref[0]; dcfg.r1 = dref[1];
            dcfg.x0 = (dref[0] < 0 || (z && dref[0] == 0)) ? 0 : dmx[0]; dcfg.y0 = (dref[0] < 0 || (z && dref[0] == 0)) ? 0 : dmy[0];
            dcfg.x1 = (dref[1] < 0 || (z && dref[1] == 0)) ? 0 : dmx[1]; dcfg.y1 = (dref[1] < 0 || (z && dref[1] == 0)) ? 0 : dmy[1];
        }
            }
            probed = false;
            if (!d_avail) continue;
            b_predict(k, c, dcfg, biwv, dpred, dcpred);
            if (k.direct_auto) {
                probed = mb_probe_skip_pred(c, cz, dpred, b_cenc, dcpred, q_lp, q_cp, nro);
                if (probed) { if (tmp) ds_t++; else ds_s++; }
            }
        }
        if constexpr (PMEMO) { pm_dv = d_avail; pm_dl = dpred; pm_dc = dcpred; }          // (--direct auto: the slice's own mode is the last pass)
        // ---- B_SKIP when the direct prediction's distortion alone undercuts the cheapest coded macroblock ----
        bool try_skip = false;
        if constexpr (NORD) {
            // analysis without RD (x264 below --subme 7 in B slices): x264_macroblock_probe_bskip on the direct prediction; from subme 3 on the skip
            // also wants both lists' first 16x16 searches to land on the direct vectors (try_skip), below it the probe decides
            // (--direct auto: the probe of the slice's mode above stands and decides alone; no direct prediction: no skip)
            bool b_skip_now = false;
            if (d_avail && !k.direct_auto) { try_skip = mb_probe_skip_pred(c, cz, dpred, b_cenc, dcpred, q_lp, q_cp, nro); b_skip_now = c.subme < 3 && try_skip; }
            else if (d_avail) b_skip_now = probed;
            pf.mark(PH_PSKIP);
            if (b_skip_now) {
                for (int ri = 0; ri < k.nref + k.nref1; ri++)
                    if (lane == 0) { int16_t *mo = (ri == 0 ? k.mv16_cur : k.mvr[ri]) + ((size_t)s * k.nmb + mbi) * 2; mo[0] = 0; mo[1] = 0; }
                direct_cand(X264GPU_MB_B_SKIP); e_t8 = 0;
                b_type = X264GPU_MB_B_SKIP; commit = true; go = true;
                break;
            }
        } else {
        {
            int e4, e8;
            psy_energy_z(cz, lane, e4, e8); fenc_e4 = wave_sum(e4) >> 1; fenc_e8 = wave_sum(e8) >> 2;
            if (d_avail) {
            int dist = wave_sum(ssd4_u8(cz, dpred));
            if (k.psy_rd_q8) {
                psy_energy_z(dpred, lane, e4, e8);
                const int d4 = wave_sum(e4) >> 1, d8 = wave_sum(e8) >> 2;
                dist += (((abs(d4 - fenc_e4) + abs(d8 - fenc_e8)) >> 1) * k.psy_rd_q8 * c.lambda + 128) >> 8;
            }
            dist += (int)(((long long)wave_sum(lane < 32 ? ssd4_u8(b_cenc, dcpred) : 0) * chroma_l2off + 128) >> 8);
            bskip_cost = uni(dist);
            }
        }
        pf.mark(PH_PSKIP);            // (MB_PROF: the direct prediction and its distortion)
        if (bskip_cost <= ((6 * lambda2 + 128) >> 8)) {
            for (int ri = 0; ri < k.nref + k.nref1; ri++)
                if (lane == 0) { int16_t *mo = (ri == 0 ? k.mv16_cur : k.mvr[ri]) + ((size_t)s * k.nmb + mbi) * 2; mo[0] = 0; mo[1] = 0; }
            direct_cand(X264GPU_MB_B_SKIP); e_t8 = 0;
            b_type = X264GPU_MB_B_SKIP; commit = true; go = true;
            break;
        }
        }
        // ---- SATD cost of the direct prediction, per 8x8 block (x264_mb_analyse_inter_direct) ----
        if (d_avail) {
            const int hs = row16_sum(cmp4(cz, dpred));
            int hc = 0;
            if (c.chroma_me) hc = quad_sum(lane < 32 ? cmp4(b_cenc, dcpred) : 0);
            cost16direct = c.lambda * 1;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int ci = rl(hs, 16 * i) + (c.chroma_me ? rl(hc, 4 * i) + rl(hc, 16 + 4 * i) : 0);
                cost16direct += ci;
                const int cd = ci + c.lambda * 1;          // + the sub-macroblock type
                if (i == 0) cost8d_0 = cd; else if (i == 1) cost8d_1 = cd; else if (i == 2) cost8d_2 = cd; else cost8d_3 = cd;
            }
        }
        // ---- 16x16 searches (x264_mb_analyse_inter_b16x16): list 1 first, every reference.  With try_skip the order is list 1 reference 0, list 0
        //      reference 0, "both within 1 of the direct vectors of block 0 -> B_SKIP", the rest of list 0, the rest of list 1 ----
        const bool t1 = k.temporal && mbx < k.mbw - 1, t2 = k.temporal && mby < k.mbh - 1;
        wl(S.cost, lane, ME_16, 0x7fffffff); wl(S.cost, lane, ME_16 + 16, 0x7fffffff);
        {
            int hthr0 = 0x7fffffff, hthr1 = 0x7fffffff;
            bool list1_skipped = false, found_skip = false;
            for (int l = 1; l >= 0 && !found_skip;) {
                const int nl = l ? k.nref1 : k.nref;
                int r = (list1_skipped && l == 1) ? 1 : 0;
                for (; r < nl; r++) {
                    if (try_skip && l == 1 && r > 0) { list1_skipped = true; break; }
                    const int ri = l ? k.nref + r : r;
                    // candidates (x264_mb_predict_mv_ref16x16): [the direct vector of the last 8x8 block if it points into this reference] [lookahead]
                    // left top top-left top-right [co-located, its right / lower neighbour scaled by the POC distances]
                    const int16_t *mvrp = (ri == 0 ? k.mv16_cur : k.mvr[ri]) + (size_t)s * k.nmb * 2;
                    const bool has_d = d_avail && rl(l ? dcfg.r1 : dcfg.r0, 48) == r;          // (h->mb.cache.ref[l][scan8[12]]: the direct prediction's last block)
                    const int16_t *lrp = l ? k.lowres_mv1 : k.lowres_mv;
                    const bool has_lr = r == 0 && lrp && (lrp + (size_t)s * k.nmb * 2)[0] != 0x7fff;
                    const int base = (has_d ? 1 : 0) + (has_lr ? 1 : 0), q = lane - base;
                    int vx = 0, vy = 0;
                    if (has_d && lane == 0) { vx = rl(l ? dcfg.x1 : dcfg.x0, 48); vy = rl(l ? dcfg.y1 : dcfg.y0, 48); }
                    else if (has_lr && lane == (has_d ? 1 : 0)) { const int16_t *lm = lrp + (size_t)s * k.nmb * 2; vx = lm[2 * mbi] * 2; vy = lm[2 * mbi + 1] * 2; }
                    else if (q >= 0 && q < 4) {
                        const int nb = q == 0 ? (left ? mbi - 1 : -1) : q == 1 ? (top ? mbi - k.mbw : -1) : q == 2 ? (topleft ? mbi - k.mbw - 1 : -1) : (topright ? mbi - k.mbw + 1 : -1);
                        if (nb >= 0) { vx = mvrp[2 * nb]; vy = mvrp[2 * nb + 1]; }
                    } else if (q >= 4 && q < 7 && k.temporal) {
                        const int16_t *l0 = k.mv16_ref0 + (size_t)s * k.nmb * 2;
                        const int scale = k.tscale[ri], jx = q - 4;
                        const bool ok = jx == 0 || (jx == 1 && (t1 || t2)) || (jx == 2 && t1 && t2);
                        const int at = jx == 0 ? mbi : (jx == 1 && t1) ? mbi + 1 : mbi + k.mbw;
                        if (ok) { vx = (l0[2 * at] * scale + 128) >> 8; vy = (l0[2 * at + 1] * scale + 128) >> 8; }
                    }
                    if (has_d) { const int dvx = rl(l ? dcfg.x1 : dcfg.x0, 48), dvy = rl(l ? dcfg.y1 : dcfg.y0, 48); if (lane == 0) { vx = dvx; vy = dvy; } }
                    S.inx = vx; S.iny = vy;
                    const int n_mvc = base + 4 + (k.temporal ? 1 + (t1 ? 1 : 0) + (t2 ? 1 : 0) : 0);
                    const int rc = refcost_l(l, r);          // (unlike the P search, x264's B search does not move the half-pel threshold by the reference cost)
                    int mvx, mvy, cost, cost_mv, px, py;
                    int thr = l ? hthr1 : hthr0;
                    search_b(l, r, D_16x16, 0, 0, 2, 2, n_mvc, early_term && nl > 1, thr, mvx, mvy, cost, cost_mv, px, py);
                    if (l) hthr1 = thr; else hthr0 = thr;
                    if (lane == 0) { int16_t *mo = (ri == 0 ? k.mv16_cur : k.mvr[ri]) + ((size_t)s * k.nmb + mbi) * 2; mo[0] = (int16_t)mvx; mo[1] = (int16_t)mvy; }
                    wl(S.mvcx, lane, 32 * l + r * 5, mvx); wl(S.mvcy, lane, 32 * l + r * 5, mvy);
                    cost += rc;
                    if (cost < rl(S.cost, ME_16 + 16 * l)) me_store(S, lane, ME_16 + 16 * l, mvx, mvy, cost, cost_mv, r, rc, px, py);
                    if (NORD && r == 0 && try_skip) {
                        const int dx = rl(l ? dcfg.x1 : dcfg.x0, 0), dy = rl(l ? dcfg.y1 : dcfg.y0, 0);
                        if (abs(rl(S.mvx, ME_16 + 16 * l) - dx) + abs(rl(S.mvy, ME_16 + 16 * l) - dy) > 1) try_skip = false;
                        else if (!l) { found_skip = true; break; }          // (the skip itself was probed before)
                    }
                }
                if (found_skip) break;
                if (list1_skipped && l == 1 && r == k.nref1) break;
                if (list1_skipped && l == 0) l = 1; else l--;
            }
            if (found_skip) {
                // B_SKIP: the references above 0 of both lists leave zero vectors for the neighbours' candidates
                for (int ri = 1; ri < k.nref + k.nref1; ri++)
                    if (ri != k.nref && lane == 0) { int16_t *mo = k.mvr[ri] + ((size_t)s * k.nmb + mbi) * 2; mo[0] = 0; mo[1] = 0; }
                direct_cand(X264GPU_MB_B_SKIP); e_t8 = 0;
                b_type = X264GPU_MB_B_SKIP; commit = true; go = true;
                break;
            }
        }
        // ---- the bi-predictive 16x16: both lists' winners averaged; the zero vectors are always tried ----
        {
            BCfg g;
            g.r0 = rl(S.ref, 0); g.x0 = rl(S.mvx, 0); g.y0 = rl(S.mvy, 0); g.r1 = rl(S.ref, 16); g.x1 = rl(S.mvx, 16); g.y1 = rl(S.mvy, 16);
            const int refc = rl(S.refcost, 0) + rl(S.refcost, 16);
            int cmv0 = rl(S.costmv, 0), cmv1 = rl(S.costmv, 16), csat;
            if constexpr (PMEMO) {
                // the probe's trip to memory fills the memo: the L0, L1 and BI candidates and the winner's later encodes ask for these rows again
                // (bi_satd(g, 15u, csat) with the rows kept)
                uint32_t pred, cpred;
                b_fetch(k, c, g, pm_l0, pm_l1, pm_c0, pm_c1);
                pm_ref = ((unsigned)g.r0 & 0xffu) | (((unsigned)g.r1 & 0xffu) << 8);
                pm_k0 = ((unsigned)g.x0 & 0xffffu) | ((unsigned)g.y0 << 16); pm_k1 = ((unsigned)g.x1 & 0xffffu) | ((unsigned)g.y1 << 16);
                b_combine(c, g, biwv, pm_l0, pm_l1, pm_c0, pm_c1, pred, cpred);
                csat = c.chroma_me ? wave_sum(lane < 32 ? cmp4(b_cenc, cpred) : 0) : 0;
                cost16bi = wave_sum(cmp4(cz, pred)) + refc + cmv0 + cmv1 + csat;
            } else cost16bi = bi_satd(g, 15u, csat) + refc + cmv0 + cmv1 + csat;
            if (g.x0 | g.y0 | g.x1 | g.y1) {
                const int l0c = (int)c.cost_base[MVCOST_HALF - rl(S.mvpx, 0)] + (int)c.cost_base[MVCOST_HALF - rl(S.mvpy, 0)];
                const int l1c = (int)c.cost_base[MVCOST_HALF - rl(S.mvpx, 16)] + (int)c.cost_base[MVCOST_HALF - rl(S.mvpy, 16)];
                BCfg z = g;
                z.x0 = z.y0 = z.x1 = z.y1 = 0;
                int cost00 = bi_satd(z, 15u, csat) + refc + l0c + l1c;
                if (c.chroma_me && cost00 < cost16bi) cost00 += csat;
                if (cost00 < cost16bi) { g = z; cmv0 = l0c; cmv1 = l1c; cost16bi = cost00; }
            }
            me_store(S, lane, 32, g.x0, g.y0, 0, cmv0, g.r0, rl(S.refcost, 0), rl(S.mvpx, 0), rl(S.mvpy, 0));
            me_store(S, lane, 48, g.x1, g.y1, 0, cmv1, g.r1, rl(S.refcost, 16), rl(S.mvpx, 16), rl(S.mvpy, 16));
            cost16bi += c.lambda * 5;
            S.cost += (lane == 0 || lane == 16) ? c.lambda * 3 : 0;
        }
        // best 16x16 type on SATD cost; the early RD pass when direct is close
        b_use16 = 0; b_type = X264GPU_MB_B_INTER; b_part = D_16x16; i_cost = rl(S.cost, 0);
        if (rl(S.cost, 16) < i_cost) { i_cost = rl(S.cost, 16); b_use16 = 1; }
        if (cost16bi < i_cost) { i_cost = cost16bi; b_use16 = 2; }
        if (cost16direct < i_cost) { i_cost = cost16direct; b_type = X264GPU_MB_B_DIRECT; }
        rd_thresh = early_term ? i_cost * (17 + (k.psy_rd_q8 != 0)) / 16 + 1 : MB_COST_MAX;
        if (NORD || !(early_term && cost16direct <= i_cost * 33 / 32)) rd_ph = 5;        // no early pass: on to the partitions
        continue;
    }
    if (rd_ph == 1 || rd_ph == 7) { go = d_avail && rd_dir == MB_COST_MAX; if (go) { direct_cand(X264GPU_MB_B_DIRECT); e_t8 = 0; } }
    else if (rd_ph == 2 || rd_ph == 8) { go = rl(S.cost, 0) < rd_thresh && rd_l0 == MB_COST_MAX; if (go) { use16_cfg(0); e_t8 = 0; } }
    else if (rd_ph == 3 || rd_ph == 9) { go = rl(S.cost, 16) < rd_thresh && rd_l1 == MB_COST_MAX; if (go) { use16_cfg(1); e_t8 = 0; } }
    else if (rd_ph == 4 || rd_ph == 10) { go = cost16bi < rd_thresh && rd_bi == MB_COST_MAX; if (go) { use16_cfg(2); e_t8 = 0; } }
    else if (rd_ph == 5) {
        if (!NORD && bskip_cost < rd_dir && bskip_cost < rd_bi && bskip_cost < rd_l0 && bskip_cost < rd_l1) {
            direct_cand(X264GPU_MB_B_SKIP); e_t8 = 0; b_type = X264GPU_MB_B_SKIP; commit = true; go = true;
        }
    } else if (rd_ph == 6) {
        if (parts & 1) {
#include "k_mb_b_parts.inc"
        }
        rd_satd_inter = i_cost;
        rd_thresh = early_term ? i_cost * (17 + (k.psy_rd_q8 != 0)) / 16 + 1 : MB_COST_MAX;
        if constexpr (NORD) {
            // ---- analysis without RD: x264_me_refine_qpel of the winner's vectors, intra on SATD cost, then phase 18 (x264_refine_bidir, final pass) ----
            // (one call site of the search: job jn = block or half jn >> 1 in list jn & 1)
            if (c.subme && b_type != X264GPU_MB_B_DIRECT) {
                for (int jn = 0; jn < 8; jn++) {
                    const int i = jn >> 1, l = jn & 1;
                    int use, slot, W = 16, H = 16, ox = 0, oy = 0, cin;
                    if (b_part == D_16x16) {
                        // (the 16x16 costs shed the macroblock type before the refinement; the bi-predictive pair refines each vector from its list's own cost)
                        if (i) break;
                        use = b_use16; slot = (use == 2 ? 32 : ME_16) + 16 * l;
                        cin = rl(S.cost, ME_16 + 16 * l) - c.lambda * 3 - rl(S.refcost, ME_16 + 16 * l);
                    } else if (b_part == D_8x8) {
                        use = i == 0 ? sub8_0 : i == 1 ? sub8_1 : i == 2 ? sub8_2 : sub8_3; slot = ME_8 + i + 16 * l;
                        W = 8; H = 8; ox = 8 * (i & 1); oy = 8 * (i >> 1);
                        cin = rl(S.cost, slot) - rl(S.refcost, slot);
                    } else {
                        if (i >= 2) break;
                        const bool hor = b_part == D_16x8;
                        use = hor ? (i ? p16x8_1 : p16x8_0) : (i ? p8x16_1 : p8x16_0); slot = (hor ? ME_16x8 : ME_8x16) + i + 16 * l;
                        W = hor ? 16 : 8; H = hor ? 8 : 16; ox = hor ? 0 : 8 * i; oy = hor ? 8 * i : 0;
                        cin = rl(S.cost, slot) - rl(S.refcost, slot);
                    }
                    if (use == 3 || use == 1 - l) continue;          // a direct block, or the other list alone
                    MeJob jb;
                    jb.search = false; jb.use_thresh = false; jb.n_mvc = 0;
                    jb.W = W; jb.H = H; jb.ox = ox; jb.oy = oy; jb.ref = l ? k.nref + rl(S.ref, slot) : rl(S.ref, slot);
                    jb.mvpx = rl(S.mvpx, slot); jb.mvpy = rl(S.mvpy, slot);
                    jb.hp_it = c.subme == 1 ? 1 : 0;                  // subpel_iterations[subme][0..1]
                    jb.qp_it = c.subme == 1 ? 1 : c.subme >= 2 && c.subme <= 5 ? (c.subme == 2 ? 1 : 2) : 0;
                    int mvx = rl(S.mvx, slot), mvy = rl(S.mvy, slot), cost = cin, cost_mv = rl(S.costmv, slot), thr = 0x7fffffff;
                    lds_sync();
                    me_search<M, ME, false>(k, L, c, jb, mvx, mvy, cost, cost_mv, thr, S, wt, pf);
                    lds_sync();
                    wl(S.mvx, lane, slot, mvx); wl(S.mvy, lane, slot, mvy); wl(S.cost, lane, slot, cost); wl(S.costmv, lane, slot, cost_mv);
                    if (b_part == D_16x16 && use != 2) i_cost = cost + c.lambda * 3;
                }
            }
            pf.mark(PH_ME_GLUE);
            satd_chroma = mb_intra_chroma_cost(k, L, c, predc);
            mb_analyse_intra<M, RD != 5 && RD != 6>(k, L, c, cz, t4, parts, c.chroma_me ? i_cost - satd_chroma : i_cost, fast_intra, early_term, false, q_li, q8i, IR, pf, (const TrCtx *)nullptr);
            if (c.chroma_me) { IR.satd_i16 += satd_chroma; IR.satd_i8 += satd_chroma; IR.satd_i4 += satd_chroma; }
            pf.mark(PH_INTRA);
            rd_best = i_cost; rd_i16 = IR.satd_i16; rd_i8 = IR.satd_i8; rd_i4 = IR.satd_i4;
            rd_t8 = -1;                // x264_mb_analyse_transform: SA8D against SATD of the prediction error decides in the encode stage
            rd_ph = 17;
            continue;
        }
    }
    else if (rd_ph == 11) { go = cost8x8bi < rd_thresh; if (go) { shape_cfg(D_8x8); e_t8 = 0; } }
    else if (rd_ph == 12) { go = cost16x8bi < rd_thresh; if (go) { shape_cfg(D_16x8); e_t8 = 0; } }
    else if (rd_ph == 13) { go = cost8x16bi < rd_thresh; if (go) { shape_cfg(D_8x16); e_t8 = 0; } }
    else if (rd_ph == 14) {
        // the decision among the inter types on RD cost, B_SKIP included
        b_type = X264GPU_MB_B_SKIP; rd_best = bskip_cost; b_part = D_16x16;
        if (rd_l0 < rd_best) { rd_best = rd_l0; b_type = X264GPU_MB_B_INTER; b_use16 = 0; }
        if (rd_l1 < rd_best) { rd_best = rd_l1; b_type = X264GPU_MB_B_INTER; b_use16 = 1; }
        if (rd_bi < rd_best) { rd_best = rd_bi; b_type = X264GPU_MB_B_INTER; b_use16 = 2; }
        if (rd_dir < rd_best) { rd_best = rd_dir; b_type = X264GPU_MB_B_DIRECT; }
        if (rd_16x8 < rd_best) { rd_best = rd_16x8; b_type = X264GPU_MB_B_INTER; b_part = D_16x8; }
        if (rd_8x16 < rd_best) { rd_best = rd_8x16; b_type = X264GPU_MB_B_INTER; b_part = D_8x16; }
        if (rd_8x8 < rd_best) { rd_best = rd_8x8; b_type = X264GPU_MB_B_8x8; b_part = D_8x8; }
        rd_t8 = 0;
        // intra analysis against the inter SATD cost (the chroma mode first: its cost rides along under chroma-ME)
        pf.mark(PH_ME_GLUE);
        satd_chroma = mb_intra_chroma_cost(k, L, c, predc, rf_dirc);
        TRC tra_ctx;                   // --trellis 2: the analysis' block encodes run the search too
        if constexpr (PSY) tr_psy_init(tra_ctx, psy_fd, k.psy_trellis);
        tra_ctx.on = 0; tra_ctx.r = 0; tra_ctx.r8 = 0; tra_ctx.model = 0; tra_ctx.tt.size_unary = nullptr; tra_ctx.tt.trans_unary = nullptr; tra_ctx.tt.lambda2 = nullptr;
        if constexpr (TRL2) {
            if (k.trellis & 64) { tra_ctx.on = k.trellis & 63; tra_ctx.r = cab.r; tra_ctx.r8 = cab.r8; tra_ctx.model = cab_modelv; tra_ctx.tt.size_unary = k.tr_su; tra_ctx.tt.trans_unary = k.tr_tu; tra_ctx.tt.lambda2 = k.tr_l2; }
        }
        mb_analyse_intra<M, RD != 5 && RD != 6>(k, L, c, cz, t4, parts, c.chroma_me ? rd_satd_inter - satd_chroma : rd_satd_inter, fast_intra, early_term, true, q_li, q8i, IR, pf, TRL2 && tra_ctx.on ? &tra_ctx : nullptr);
        if (c.chroma_me) { IR.satd_i16 += satd_chroma; IR.satd_i8 += satd_chroma; IR.satd_i4 += satd_chroma; }
        pf.mark(PH_INTRA);
        // x264_mb_analyse_transform_rd: the other transform size for the winner (B_SKIP has none)
        go = b_type != X264GPU_MB_B_SKIP && k.dct8x8;
        if (go) { winner_cfg(); e_t8 = 1; }
    } else if (rd_ph == 15) {
        rd_ithresh = !early_term ? MB_COST_MAX : rd_satd_inter * 17 / 16 + 1;
        go = IR.satd_i16 < rd_ithresh; e_type = X264GPU_MB_I16x16;
    } else if (rd_ph == 16) { go = IR.satd_i4 < rd_ithresh; e_type = X264GPU_MB_I4x4; }
    else if (rd_ph == 17) { go = IR.satd_i8 < rd_ithresh; e_type = X264GPU_MB_I8x8; }
    else if (rd_ph >= 18) {
        bool fresh = true;
        if constexpr (REF) fresh = !rf_on;          // (rf_on here: the inter refinement's coroutine is under way, k_mb_b_rdrefine.inc below)
        if (fresh) {
        int best = rd_best;
        int ft = b_type;
        if (rd_i16 < best) { best = rd_i16; ft = X264GPU_MB_I16x16; }
        if (rd_i8 < best) { best = rd_i8; ft = X264GPU_MB_I8x8; }
        if (rd_i4 < best) { best = rd_i4; ft = X264GPU_MB_I4x4; }
        i_cost = best;
        if (ft < X264GPU_MB_P_L0) {
            e_type = ft; if (lane == 0) recd.cost = i_cost;
            if constexpr (REF) {
                // x264_macroblock_analyse, B slices at --subme 9 (i_mbrd 2): intra_rd_refine of the chosen intra type
                const int sites = (k.rd >> 1) & 31;
                if (c.subme >= 9 && (sites & 30)) {
                    rf_on = true; rf_kind = 1; rf_st = 0; rf_part = 0; rf_wait = 0; rf_done = 0; rf_amvd = 0; rf_pk = 0;
                    break;
                }
            }
        }
        else {
            pf.mark(PH_ME_GLUE);
            // x264_refine_bidir (subme >= 5): the winner's bi-predicted partitions refine both vectors together on SATD
            if (c.subme >= 5 && b_type == X264GPU_MB_B_INTER && b_part == D_16x16 && b_use16 == 2) {
#define BIREF_SLOT 32
#define BIREF_W 16
#define BIREF_H 16
#define BIREF_OX 0
#define BIREF_OY 0
#include "k_mb_b_refine.inc"
            } else if (c.subme >= 5 && (b_type == X264GPU_MB_B_INTER || b_type == X264GPU_MB_B_8x8) && b_part != D_16x16) {
                const int np = b_part == D_8x8 ? 4 : 2;
                for (int kp = 0; kp < np; kp++) {
                    const int use = b_part == D_8x8 ? (kp == 0 ? sub8_0 : kp == 1 ? sub8_1 : kp == 2 ? sub8_2 : sub8_3) : b_part == D_16x8 ? (kp ? p16x8_1 : p16x8_0) : (kp ? p8x16_1 : p8x16_0);
                    if (use != 2) continue;
                    const int bslot = (b_part == D_8x8 ? ME_8 : b_part == D_16x8 ? ME_16x8 : ME_8x16) + kp;
                    const int bw = b_part == D_16x8 ? 16 : 8, bh = b_part == D_8x16 ? 16 : 8;
                    const int box = b_part == D_8x16 ? 8 * kp : b_part == D_8x8 ? 8 * (kp & 1) : 0, boy = b_part == D_16x8 ? 8 * kp : b_part == D_8x8 ? 8 * (kp >> 1) : 0;
#define BIREF_SLOT bslot
#define BIREF_W bw
#define BIREF_H bh
#define BIREF_OX box
#define BIREF_OY boy
#include "k_mb_b_refine.inc"
                }
            }
            pf.mark(PH_INTRA_CHROMA);        // (MB_PROF, B slices: the bidirectional refinement)
            winner_cfg();
            e_t8 = rd_t8;
            if constexpr (REF) {
                // x264_macroblock_analyse, B slices at --subme 9 (i_mbrd 2): the chosen inter type's vectors once more on RD cost
                if (c.subme >= 9 && ((k.rd >> 1) & 1) && (b_type == X264GPU_MB_B_INTER || b_type == X264GPU_MB_B_8x8)) {
                    rf_on = true; rf_kind = 2; rf_st = 0; rf_part = 0; rf_wait = 0; rf_done = 0; rf_amvd = 0; rf_amvd1 = 0; rf_pk = 0;
                }
            }
        }
        if (!rf_on) { commit = true; go = true; }
        }
        if constexpr (REF) {
            if (rf_on && rf_kind == 2) {
#include "k_mb_b_rdrefine.inc"
            }
        }
    }
    if (go) break;
}

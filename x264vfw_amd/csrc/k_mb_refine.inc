// k_mb_refine.inc — RD refinement of the macroblock type the RD decision chose (x264 --subme 8 and up, i_mbrd >= 2: [x264-upstream] encoder/me.c
// x264_me_refine_qpel_rd, encoder/analyse.c intra_rd_refine and their hooks in x264_macroblock_analyse; restates oracle/analyse.c
// refine_inter_p_rd / me_refine_qpel_rd / intra_rd_refine).  Included inside k_mb_slice's pass loop (REF instantiations), entered at the top of a
// pass while rd_ph == 9: a coroutine that hands ONE candidate at a time to the encode + pricing stages below (rf_pk says what kind of pass:
// 0 the whole macroblock, 1 an inter part, 2 an Intra_4x4 block, 3 an Intra_8x8 block, 4 the chroma of an intra macroblock), gets the cost back in
// rf_cost (rf_wait), and ends with the final pass (commit).
//
// Inter (rf_kind 0): per part of the chosen P type, in order — SATD of the start vector, [RD cost of it], the predicted vector, a sub-pel
// hexagon (six points, then half hexagons away from where it came from, up to nine times), a square of eight; every candidate is first costed
// on SATD + vector bits and only priced on RD cost when that is within 17/16 of the best SATD so far.
for (;;) {
    if (rf_kind == 0) {
        const int np = e_part == D_16x16 ? 1 : e_part == D_8x8 ? 4 : 2;
        if (rf_wait) {
            // the cost of candidate (rf_cx, rf_cy) came back
            rf_wait = 0;
            rf_lmx = abs(rf_cx - rf_mvpx); rf_lmy = abs(rf_cy - rf_mvpy); rf_priced = 1;
            if (rf_cost < rf_bcost) { rf_bcost = rf_cost; rf_bmx = rf_cx; rf_bmy = rf_cy; if (rf_cdir != -99) rf_dir = rf_cdir; }
        }
        int cx = 0, cy = 0, cdir = -99;
        bool have = false, avoid = true, force_rd = false, no_rd = false;
        if (rf_st == 0) {
            // ---- set up the part ----
            rf_slot = e_part == D_16x16 ? ME_16 : e_part == D_16x8 ? ME_16x8 + rf_part : e_part == D_8x16 ? ME_8x16 + rf_part : ME_8 + rf_part;
            rf_b0 = e_part == D_16x8 ? 2 * rf_part : rf_part;
            rf_b1 = e_part == D_16x8 ? rf_b0 + 1 : e_part == D_8x16 ? rf_b0 + 2 : -1;
            rf_pm8 = e_part == D_16x16 ? 15 : (1 << rf_b0) | (rf_b1 >= 0 ? 1 << rf_b1 : 0);
            rf_ref = rl(S.ref, rf_slot);
            rf_mv0x = rl(S.mvx, rf_slot); rf_mv0y = rl(S.mvy, rf_slot);
            rf_mvpx = rl(S.mvpx, rf_slot); rf_mvpy = rl(S.mvpy, rf_slot);
            if (e_part != D_16x16 && rf_part != 0) {
                // the parts refined before this one moved: predict again (the cache holds their final vectors, nothing of the parts to come)
                const int x8 = rf_b0 & 1, y8 = rf_b0 >> 1, g0 = (y8 + 1) * 4 + x8 + 1;
                const int w8 = e_part == D_16x8 ? 2 : 1, h8 = e_part == D_8x16 ? 2 : 1;
                const int sv = S.cref;
                const bool mine = lane == g0 || (w8 == 2 && lane == g0 + 1) || (h8 == 2 && lane == g0 + 4);
                S.cref = mine ? rf_ref : S.cref;                      // the part's own reference is cached before its vector is predicted
                mb_predict_mv(S, e_part, x8, y8, w8, rf_ref, rf_mvpx, rf_mvpy);
                S.cref = sv;
            }
            rf_pmx = rf_mvpx; rf_pmy = rf_mvpy;
            rf_bmx = rf_mv0x; rf_bmy = rf_mv0y; rf_bcost = ~0ull; rf_bsatd = MB_COST_MAX; rf_dir = -2; rf_pmvchk = 0; rf_priced = 0;
            if (k.psy_rd_q8 && e_part != D_16x16) {
                // cached_hadamard of the source over the part
                int e4, e8;
                psy_energy_z(cz, lane, e4, e8);
                rf_f4 = wave_sum(((rf_pm8 >> (lane >> 4)) & 1) ? e4 : 0) >> 1;
                rf_f8 = wave_sum((lane < 32 && ((rf_pm8 >> (lane >> 3)) & 1)) ? e8 : 0) >> 2;
            }
            cx = rf_bmx; cy = rf_bmy; have = true; avoid = false;
            if (e_part == D_16x16) { no_rd = true; rf_bcost = (unsigned long long)(unsigned)i_cost; } else force_rd = true;
            rf_st = 1;
        } else if (rf_st == 1) {
            // ---- the predicted vector ----
            rf_st = 2;
            if ((rf_bmx != rf_pmx || rf_bmy != rf_pmy) && rf_pmx >= c.smin0 && rf_pmx <= c.smax0 && rf_pmy >= c.smin1 && rf_pmy <= c.smax1) {
                cx = rf_pmx; cy = rf_pmy; have = true; avoid = false; rf_pmvchk = 1;
            }
        } else if (rf_st == 2) {
            // the hexagon never repeats its centre: if the predictor won, the vector to avoid becomes the old one
            if (rf_pmvchk && rf_bmx == rf_pmx && rf_bmy == rf_pmy) { rf_pmx = rf_mv0x; rf_pmy = rf_mv0y; }
            if (rf_bmy < c.smin1 + 3 || rf_bmy > c.smax1 - 3 || rf_bmx < c.smin0 + 3 || rf_bmx > c.smax0 - 3) { rf_bmx = rf_mv0x; rf_bmy = rf_mv0y; rf_st = 7; }      // too close to the limits: the part keeps its vector
            else { rf_st = 3; rf_j = 0; rf_dir = -2; rf_omx = rf_bmx; rf_omy = rf_bmy; }
        } else if (rf_st == 3) {
            // ---- sub-pel hexagon: (-2,0) (-1,2) (1,2) (2,0) (1,-2) (-1,-2) ----
            if (rf_j < 6) { cx = rf_omx + hex_dx(rf_j + 1); cy = rf_omy + hex_dy(rf_j + 1); cdir = rf_j; have = true; rf_j++; }
            else if (rf_dir != -2) { rf_st = 4; rf_i = 1; rf_j = 3; }
            else rf_st = 5;
        } else if (rf_st == 4) {
            // ---- half hexagons that do not overlap the previous one ----
            if (rf_j == 3) {
                // a new iteration
                if (rf_i >= 10 || (rf_i > 1 && rf_dir == -2) || rf_bmy < c.smin1 + 3 || rf_bmy > c.smax1 - 3) rf_st = 5;
                else { rf_odir = rf_dir == -1 ? 5 : rf_dir == 6 ? 0 : rf_dir; rf_dir = -2; rf_omx = rf_bmx; rf_omy = rf_bmy; rf_j = 0; rf_i++; }      // mod6m1[dir + 1]
            } else { cx = rf_omx + hex_dx(rf_odir + rf_j); cy = rf_omy + hex_dy(rf_odir + rf_j); cdir = rf_odir - 1 + rf_j; have = true; rf_j++; }
        } else if (rf_st == 5) { rf_st = 6; rf_j = 0; rf_omx = rf_bmx; rf_omy = rf_bmy; }
        else if (rf_st == 6) {
            // ---- square refine ----
            if (rf_j < 8) { cx = rf_omx + sq_dx(rf_j + 1); cy = rf_omy + sq_dy(rf_j + 1); cdir = 0; have = true; rf_j++; }
            else { rf_lmx = abs(rf_bmx - rf_mvpx); rf_lmy = abs(rf_bmy - rf_mvpy); rf_priced = 1; rf_st = 7; }
        } else {
            // ---- the part is done: its vector into the search results and the cache, its |mvd| for the parts after it ----
            wl(S.mvx, lane, rf_slot, rf_bmx); wl(S.mvy, lane, rf_slot, rf_bmy);
            if (e_part != D_16x16) {
                const int w8 = e_part == D_16x8 ? 2 : 1, h8 = e_part == D_8x16 ? 2 : 1;
                for (int t = 0; t < 2; t++) {
                    const int b8 = t ? rf_b1 : rf_b0;
                    if (b8 < 0) continue;
                    const int g = ((b8 >> 1) + 1) * 4 + (b8 & 1) + 1;
                    wl(S.cref, lane, g, rf_ref); wl(S.cmvx, lane, g, rf_bmx); wl(S.cmvy, lane, g, rf_bmy);
                    if (rf_priced) {
                        rf_amvd &= ~(0xffffull << (16 * b8));
                        rf_amvd |= ((unsigned long long)min(rf_lmx, 66) | ((unsigned long long)min(rf_lmy, 66) << 8)) << (16 * b8);
                    }
                    rf_done |= 1 << b8;
                }
                (void)w8; (void)h8;
            }
            if (++rf_part < np) { rf_st = 0; continue; }
            // "in rare cases we can end up qpel-RDing our way back to a larger partition size": two halves on one vector and reference
            if (e_part == D_16x8 || e_part == D_8x16) {
                const int s0 = e_part == D_16x8 ? ME_16x8 : ME_8x16;
                if (rl(S.mvx, s0) == rl(S.mvx, s0 + 1) && rl(S.mvy, s0) == rl(S.mvy, s0 + 1) && rl(S.ref, s0) == rl(S.ref, s0 + 1)) {
                    wl(S.mvx, lane, ME_16, rl(S.mvx, s0)); wl(S.mvy, lane, ME_16, rl(S.mvy, s0)); wl(S.ref, lane, ME_16, rl(S.ref, s0));
                    e_part = D_16x16; best_part = D_16x16;
                }
            }
            rf_pk = 0; commit = true; go = true;
            break;
        }
        if (!have) continue;
        // ---- COST_MV_SATD: the prediction of the part at the candidate, SATD + vector bits ----
        int satd = MB_COST_MAX;
        if (!(avoid && cx == rf_pmx && cy == rf_pmy)) {
            uint32_t pr = mc_luma_row4(ref_plane00(k, s, rf_ref), k.plane_bytes, k.rs, c.px + zx, c.py + zy, cx, cy);
            if (k.wp_any) { const int wpk = uni(k.wl0[rf_ref]); if (wpk >> 24) pr = wp4(pr, wpk); }
            rf_pred = pr;
            satd = wave_sum(((rf_pm8 >> (lane >> 4)) & 1) ? satd4_half(cz, pr, lane) : 0)
                   + (int)c.cost_base[MVCOST_HALF + cx - rf_mvpx] + (int)c.cost_base[MVCOST_HALF + cy - rf_mvpy];
            if (satd < rf_bsatd) rf_bsatd = satd;
        }
        if (no_rd || !(force_rd || satd <= rf_bsatd + (rf_bsatd >> 4))) continue;
        // ---- COST_MV_RD: the candidate goes through the encode and pricing stages ----
        rf_cx = cx; rf_cy = cy; rf_cdir = cdir; rf_wait = 1;
        if (e_part == D_16x16) { wl(S.mvx, lane, ME_16, cx); wl(S.mvy, lane, ME_16, cy); rf_pk = 0; }
        else rf_pk = 1;
        go = true;
        break;
    } else {
        // ---- intra_rd_refine: the chosen intra type's modes once more, on RD cost.  rf_st: 0 start, 10 Intra_16x16 modes, 20 chroma modes,
        //      30 Intra_4x4 blocks, 40 Intra_8x8 blocks, 99 done ----
        const int sites = k.rd >> 1;
        TRC tra_ref;                   // --trellis 2: the refinement's block encodes run the search too (x264 b_trellis during the analysis)
        if constexpr (PSY) tr_psy_init(tra_ref, psy_fd, k.psy_trellis);
        tra_ref.on = 0; tra_ref.r = 0; tra_ref.r8 = 0; tra_ref.model = 0; tra_ref.tt.size_unary = nullptr; tra_ref.tt.trans_unary = nullptr; tra_ref.tt.lambda2 = nullptr;
        if constexpr (TRL2) {
            if (k.trellis & 64) { tra_ref.on = k.trellis & 63; tra_ref.r = cab.r; tra_ref.r8 = cab.r8; tra_ref.model = cab_modelv; tra_ref.tt.size_unary = k.tr_su; tra_ref.tt.trans_unary = k.tr_tu; tra_ref.tt.lambda2 = k.tr_l2; }
        }
        if (rf_st == 0) {
            rf_old = IR.pred16; rf_bm = IR.pred16; rf_bcost = (unsigned long long)(unsigned)i_cost; rf_j = 0;
            rf_st = e_type == X264GPU_MB_I16x16 && (sites & 2) ? 10 : 20;
        }
        if (rf_st == 10) {
            // every other available 16x16 mode whose SATD cost is within 9/8 of the chosen one's: a whole-macroblock pass each
            if (rf_wait) { rf_wait = 0; if (rf_cost < rf_bcost) { rf_bcost = rf_cost; rf_bm = rf_cm; } }
            const int n16 = left && top ? 4 : (left || top) ? 2 : 1;
            const int l0 = left && top ? PRED16_V : left ? PRED16_DC_LEFT : top ? PRED16_DC_TOP : PRED16_DC_128, l1 = left && top ? PRED16_H : left ? PRED16_H : PRED16_V;
            auto mode_at = [&](int i) { return i == 0 ? l0 : i == 1 ? l1 : i == 2 ? PRED16_DC : PRED16_P; };
            auto dir_at = [&](int i) { return i == 0 ? IR.dir16[0] : i == 1 ? IR.dir16[1] : i == 2 ? IR.dir16[2] : IR.dir16[3]; };
            int dold = MB_COST_MAX;
            for (int i = 0; i < n16; i++) if (mode_at(i) == rf_old) dold = dir_at(i);
            const int thresh = early_term ? dold * 9 / 8 : MB_COST_MAX;
            bool out = false;
            while (rf_j < n16) {
                const int m = mode_at(rf_j), d = dir_at(rf_j);
                rf_j++;
                if (m == rf_old || d > thresh || d >= MB_COST_MAX) continue;
                IR.pred16 = m; rf_cm = m; e_type = X264GPU_MB_I16x16; rf_pk = 0; rf_wait = 1; out = true;
                break;
            }
            if (out) { go = true; break; }
            IR.pred16 = rf_bm; rf_st = 20; rf_j = 0; rf_wait = 0;
        }
        if (rf_st == 20) {
            // the chroma mode: the candidates within 5/4 of the chosen one's SATD cost, chroma-only passes (rf_pk 4); first the chosen mode itself
            // (x264 recounts the bits of what intra_rd left; coding it again gives the same pixels and levels)
            const unsigned lst = left && top ? 0x3210u : left ? 0x14u : top ? 0x25u : 0x6u;
            const int nc = left && top ? 4 : (left || top) ? 2 : 1;
            if (!(sites & 4) || nc < 2) rf_st = 30;
            else {
                const int thresh = early_term ? satd_chroma * 5 / 4 : MB_COST_MAX;
                auto dirc_at = [&](int i) { return i == 0 ? rf_dirc[0] : i == 1 ? rf_dirc[1] : i == 2 ? rf_dirc[2] : rf_dirc[3]; };
                if (rf_wait) {
                    rf_wait = 0;
                    if (rf_j == 0 || rf_cost < rf_bcost) { rf_bcost = rf_cost; rf_bm = rf_cm; }
                    rf_j++;          // rf_j: 0 = the chosen mode is out, i + 1 = list entry i is out / next
                    rf_cbpc = cbp_chroma;
                } else if (rf_j == 0) {
                    // any candidate at all?
                    bool any = false;
                    for (int i = 0; i < nc; i++) any = any || (dirc_at(i) < thresh && (int)((lst >> (4 * i)) & 15) != predc);
                    if (any) { rf_cm = predc; rf_bdct = 1; rf_pk = 4; rf_wait = 1; go = true; break; }
                    rf_st = 30;
                }
                if (rf_st == 20) {
                    bool out = false;
                    while (rf_j - 1 < nc) {
                        const int i = rf_j - 1, m = (int)((lst >> (4 * i)) & 15);
                        if (dirc_at(i) < thresh && m != predc) { rf_cm = m; rf_bdct = rf_cbpc != 0; rf_pk = 4; rf_wait = 1; out = true; break; }      // (no transform once a mode without residual was seen)
                        rf_j++;
                    }
                    if (out) { go = true; break; }
                    predc = rf_bm; rf_st = 30;
                }
            }
        }
        if (rf_st == 30) { rf_st = e_type == X264GPU_MB_I4x4 && (sites & 8) ? 31 : e_type == X264GPU_MB_I8x8 && (sites & 16) ? 41 : 99; rf_i = 0; rf_j = 0; rf_wait = 0; }
        if (rf_st == 31) {
            // ---- Intra_4x4: block by block, every available mode — the candidates' encodes side by side (lane = mode * 4 + row, as the analysis
            //      costs them), then one pricing pass per mode (rf_pk 2) ----
            const int idx = rf_i, bx = z_bx(idx), by = z_by(idx);
            uint8_t *bt = L.tile + IT_ORG + by * 4 * IT_STRIDE + bx * 4;
            if (rf_wait) { rf_wait = 0; if (rf_cost < rf_bcost) { rf_bcost = rf_cost; rf_bm = rf_cm; } }
            else if (rf_j == 0) {
                const int avail = i4_avail(c.mbx, c.sy, k.mbw, idx);
                const int all3 = AVAIL_LEFT | AVAIL_TOP | AVAIL_TOPLEFT;
                const int id = (avail & all3) == all3 ? 4 : avail & (AVAIL_LEFT | AVAIL_TOP);
                rf_list = id == 4 ? 0xF876543210ull : id == 3 ? 0xF873012ull : id == 1 ? 0xF812ull : id == 2 ? 0xF7302ull : 0xF2ull;
                lds_sync();
                pred4_build_u(L.U, bt, IT_STRIDE, avail, lane);
                const uint32_t pr = pred4_row4(L.U, t4);
                const uint32_t en = (uint32_t)__shfl((int)cz, idx * 4 + j4);
                int e[4], p[4], v[4];
                unpack4(en, e); unpack4(pr, p);
#pragma unroll
                for (int t = 0; t < 4; t++) v[t] = e[t] - p[t];
                dct4_quad(v, lane);
                if (TRL2 && (tra_ref.on & TR_I4)) {
                    if (lane < 36) store_levels_scan(L.lv8 + (lane >> 2) * 16, v, j4);
                    lds_sync();
                    trellis_run<2>(tra_ref, L.lv8, 16, 9, c.qp, true, lane, tr_fd4(tra_ref) + idx * 16, 0);          // (psy: nine predictions of ONE source block)
                    lds_sync();
                    if (lane < 36) load_levels_scan(L.lv8 + (lane >> 2) * 16, v, j4);
                    lds_sync();
                } else quant4_row(v, q_li, j4);
                const bool nz = quad_or((v[0] | v[1] | v[2] | v[3]) != 0 ? 1 : 0) != 0;
                rf4_v0 = v[0]; rf4_v1 = v[1]; rf4_v2 = v[2]; rf4_v3 = v[3];
                dequant4_row(v, q_li, j4);
                idct4_quad(v, lane);
#pragma unroll
                for (int t = 0; t < 4; t++) v[t] += p[t];
                const uint32_t rz = nz ? pack4_clip(v) : pr;
                rf4_rz = rz;
                // ssd_plane( PIXEL_4x4 ): SSD + the psy term of blocks below 8x8: |SATD - SAD / 2 of the reconstruction against zero - the same of the source|
                int d = quad_sum(ssd4_u8(en, rz));
                if (k.psy_rd_q8) {
                    const int fs = quad_sum(satd4_half(en, 0u, lane)) - (quad_sum((int)__builtin_amdgcn_sad_u8(en, 0u, 0u)) >> 1);
                    const int ds = quad_sum(satd4_half(rz, 0u, lane)) - (quad_sum((int)__builtin_amdgcn_sad_u8(rz, 0u, 0u)) >> 1);
                    d += (abs(ds - fs) * k.psy_rd_q8 * c.lambda + 128) >> 8;
                }
                // distortion and non-zero flag of each mode's encode: through LDS (the search's candidate list, idle here), not a cross-lane register read —
                // in the largest instantiations the register is spilled and reloaded under a partial EXEC mask, and a readlane of an inactive lane then
                // returns what was there before (seen on MI355X: B slices, --subme 9)
                if (j4 == 0 && lane < 36) ((int *)L.cand)[lane >> 2] = (d << 1) | (nz ? 1 : 0);
                rf_bcost = ~0ull; rf_bm = L.modes4[idx]; rf_j = 1;
            }
            if ((rf_list & 15) != 15) {
                const int m = (int)(rf_list & 15);
                rf_list >>= 4;
                // this mode's levels into the level buffer, its mode into the mode cache: the pricing pass reads both
                lds_sync();
                if ((lane >> 2) == m) { int v[4] = { rf4_v0, rf4_v1, rf4_v2, rf4_v3 }; store_levels_scan(rd_lvs + idx * 16, v, j4); }
                if (lane == 0) L.modes4[idx] = (uint8_t)m;
                lds_sync();
                rf_cm = m; rf_pk = 2; rf_wait = 1; go = true;
                break;
            }
            // the block is settled: the best mode's pixels, levels, non-zero flag and mode stay
            {
                const int m = rf_bm;
                lds_sync();
                if ((lane >> 2) == m) {
                    *(uint32_t *)(bt + j4 * IT_STRIDE) = rf4_rz;
                    int v[4] = { rf4_v0, rf4_v1, rf4_v2, rf4_v3 };
                    store_levels_scan(L.lv4 + idx * 16, v, j4);
                }
                if (lane == 0) L.modes4[idx] = (uint8_t)m;
                const int bnz = ((const int *)L.cand)[m] & 1;
                IR.nnz4 = (IR.nnz4 & ~(1u << idx)) | ((unsigned)bnz << idx);
                rf_nnzc = (rf_nnzc & ~(1u << idx)) | ((unsigned)bnz << idx);
                lds_sync();
            }
            rf_j = 0;
            if (++rf_i < 16) continue;
            rf_st = 99;
        }
        if (rf_st == 41) {
            // ---- Intra_8x8: block by block, the modes whose SATD cost is within 11/8 of the chosen one's, one block-encode + pricing pass each (rf_pk 3) ----
            const int idx = rf_i;
            if (rf_wait) {
                rf_wait = 0;
                if (rf_cost < rf_bcost) {
                    rf_bcost = rf_cost; rf_bm = rf_cm; rf8_cbp = cbp_luma; rf8_n4 = nnz & (0xfu << (4 * idx));
                    // keep what the block's pass left: levels and pixels (lanes 0..7: the block's rows)
#pragma unroll
                    for (int i = 0; i < 8; i++) rf8_v[i] = rf8c_v[i];
                    rf8_blo = rf8c_lo; rf8_bhi = rf8c_hi;
                }
            } else if (rf_j == 0) {
                const int avail = i8_avail(left, top, topright, idx);
                const int all3 = AVAIL_LEFT | AVAIL_TOP | AVAIL_TOPLEFT;
                const int id = (avail & all3) == all3 ? 4 : avail & (AVAIL_LEFT | AVAIL_TOP);
                rf_list = id == 4 ? 0xF876543210ull : id == 3 ? 0xF873012ull : id == 1 ? 0xF812ull : id == 2 ? 0xF7302ull : 0xF2ull;
                rf_bcost = ~0ull; rf_bm = L.modes8[idx * 4]; rf_old = rf_bm; rf_j = 1; rf8_cbp = rf_cbp_i8; rf8_n4 = IR.nnz8 & (0xfu << (4 * idx));
            }
            {
                const int thresh = early_term ? rl(IR.dir8v, idx * 9 + rf_old) * 11 / 8 : MB_COST_MAX;
                bool out = false;
                while ((rf_list & 15) != 15) {
                    const int m = (int)(rf_list & 15);
                    rf_list >>= 4;
                    if (rl(IR.dir8v, idx * 9 + m) > thresh) continue;
                    lds_sync();
                    if (lane < 4) L.modes8[idx * 4 + lane] = (uint8_t)m;
                    lds_sync();
                    rf_cm = m; rf_pk = 3; rf_wait = 1; out = true;
                    break;
                }
                if (out) { go = true; break; }
            }
            // the block is settled: the best mode's pixels and levels back in place
            {
                const int x8 = idx & 1, y8 = idx >> 1, r8 = lane & 7;
                uint8_t *bt8 = L.tile8 + IT_ORG + y8 * 8 * IT_STRIDE + x8 * 8;
                lds_sync();
                if (lane < 8) {
                    *(uint32_t *)(bt8 + r8 * IT_STRIDE) = rf8_blo; *(uint32_t *)(bt8 + r8 * IT_STRIDE + 4) = rf8_bhi;
#pragma unroll
                    for (int i = 0; i < 8; i++) { const int z = c_zigzag8_inv[r8 * 8 + i]; L.lv8[(idx * 4 + (z & 3)) * 16 + (z >> 2)] = (int16_t)rf8_v[i]; }
                }
                if (lane < 4) L.modes8[idx * 4 + lane] = (uint8_t)rf_bm;
                rf_cbp_i8 = rf8_cbp;
                IR.nnz8 = (IR.nnz8 & ~(0xfu << (4 * idx))) | rf8_n4; IR.cbp8 = rf8_cbp;
                lds_sync();
            }
            rf_j = 0;
            if (++rf_i < 4) continue;
            rf_st = 99;
        }
        rf_pk = 0; commit = true; go = true;
        break;
    }
}

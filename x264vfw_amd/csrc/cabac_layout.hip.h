// cabac_layout.hip.h — where the device keeps the CABAC context variables of a slice (cabac_rd.hip.h codes with them, encoder.hip unpacks them
// for the tests).
#pragma once

namespace x264gpu {

// Where context variable ctx lives: register, lane, bit shift.  Registers 0 = a0 and 3 = a1: header syntax, coded_block_flags and the
// transform-size flag, ONE CONTEXT A LANE in the low byte (a0: contexts 0..63 in lanes 0..63; a1: contexts 64..104 in lanes 0..40 and
// 399..401 in lanes 41..43) — the lane that owns a context collects that context's bins of a macroblock as a string and walks them through
// the chain table (cabac_rd.hip.h cab_put / cab_walk_a), and between two cab_mb calls the rest of the dword is zero;
// 1 = r: the residual contexts of block categories 0..4, one BYTE PER CATEGORY in every lane; 2 = r8: those of 8x8 blocks.
// In r and r8 the lane is the context's ROLE: lane p = significant_coeff_flag of scan position p, lane 16 + p = last_significant_coeff_flag
// of position p, lane 32 + q = coeff_abs_level_minus1 context q (chroma DC, which shares its byte with luma DC, sits in lanes 48..63
// instead; 8x8 blocks: lane = ctxIdxInc).  All significance / last flags of a 4x4 block then code in ONE step, every lane its own context,
// and the level bins run as a loop in which only the lanes of the two contexts concerned act.
__host__ __device__ inline bool cab_locate(int ctx, int &reg, int &lane, int &sh)
{
    const int sig_off[6] = { 105, 120, 134, 149, 152, 402 }, last_off[6] = { 166, 181, 195, 210, 213, 417 }, abs_off[6] = { 227, 237, 247, 257, 266, 426 };
    const int n_sig[6] = { 15, 14, 15, 3, 14, 15 }, n_last[6] = { 15, 14, 15, 3, 14, 9 }, n_abs[6] = { 10, 10, 10, 9, 10, 10 }, byte_of[6] = { 3, 1, 0, 3, 2, 0 };
    if (ctx < 64) { reg = 0; lane = ctx; sh = 0; return true; }
    if (ctx < 105) { reg = 3; lane = ctx - 64; sh = 0; return true; }
    if (ctx >= 399 && ctx <= 401) { reg = 3; lane = ctx - 399 + 41; sh = 0; return true; }
    for (int cat = 0; cat < 6; cat++) {
        int role = -1, i = 0;
        if (ctx >= sig_off[cat] && ctx < sig_off[cat] + n_sig[cat]) { role = 0; i = ctx - sig_off[cat]; }
        else if (ctx >= last_off[cat] && ctx < last_off[cat] + n_last[cat]) { role = 1; i = ctx - last_off[cat]; }
        else if (ctx >= abs_off[cat] && ctx < abs_off[cat] + n_abs[cat]) { role = 2; i = ctx - abs_off[cat]; }
        if (role < 0) continue;
        reg = cat == 5 ? 2 : 1; sh = 8 * byte_of[cat];
        lane = cat == 3 ? (role == 0 ? 48 + i : role == 1 ? 52 + i : 55 + i) : role * 16 + i;
        return true;
    }
    return false;
}

}  // namespace x264gpu

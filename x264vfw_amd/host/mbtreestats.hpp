// mbtreestats.hpp — the macroblock-tree statistics file of a 2-pass encode (x264's second statistics file, <stats>.mbtree; [x264-upstream] encoder/ratecontrol.c
// x264_ratecontrol_new / macroblock_tree_read / x264_ratecontrol_end, common/mc.c mbtree_fix8_pack / _unpack).  The first pass writes the quantiser offsets the
// tree left with every picture kept as a reference; the second pass, which has no future pictures to run a lookahead over, reads them back.  One record a kept
// picture, coding order: a byte of slice type (P 0, B 1, I 2), then one big-endian 8.8 fixed-point word a macroblock.  Records have one size: the second pass
// seeks to the one it needs.  Opt-in for now: X264GPU_MBTREE_STATS=1 in the environment; without it 2-pass sessions run as before (mbtree 0).
#pragma once
#include "host.hpp"
#include <stdio.h>
#include <string>
#include <vector>

namespace x264host {

// the number format on the host, the device entries' arithmetic (a device library without them: the unit converts here)
uint16_t mbtree_fix8_pack(float offset);
float mbtree_fix8_unpack(uint16_t word);

struct MbTreeStats {
    bool writing = false, reading = false;          // what the session does with the file (neither: nothing of this unit runs)

    static bool opted_in();          // X264GPU_MBTREE_STATS=1
    // second pass: is the first pass' tree usable?  The statistics' header must say mbtree=1 and name the session's width x height (offsets are not rescaled), and
    // <stat_in>.mbtree must hold a record for every kept picture of the statistics.  false: one WARNING that names the cause; the session runs mbtree 0
    bool check_read(const x264_param_t &p, const char *stat_in, int nmb);
    // the device and host buffers, the file (writing: <stat_out>.mbtree.temp, reading: <stat_in>.mbtree); one INFO line says where the words are converted
    bool open(const x264_param_t &p, const char *stat_in, const char *stat_out, int nmb);
    // first pass, behind the issue of a kept picture (type PIC_*): its offsets are packed and downloaded on `stream`, the record joins the file
    bool write_record(const x264_param_t &p, int pic_type, const float *d_offsets, void *stream);
    // second pass, before a picture is issued: the record of coded picture `coded_index`, uploaded and unpacked into d_offsets on `stream`.
    // 1: done; 0: the picture has no record (not kept in the first pass, or behind its end); -1: said in the log (type mismatch, read or device failure)
    int read_record(const x264_param_t &p, long coded_index, int pic_type, float *d_offsets, void *stream);
    // x264_ratecontrol_delete: a written file takes its name
    void close(const x264_param_t &p);

private:
    FILE *file = nullptr;
    std::string path;                     // without ".temp"
    int nmb = 0;
    bool on_device = false;
    uint16_t *d_words = nullptr;          // device: one record's words
    std::vector<uint16_t> words;          // host: the same
    std::vector<float> floats;            // host conversion only
    std::vector<int> rank;                // by coding index of the statistics: the picture's place among the kept ones, -1 for a picture not kept
};

}  // namespace x264host

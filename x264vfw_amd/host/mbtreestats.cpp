// mbtreestats.cpp — the macroblock-tree statistics file of a 2-pass encode (host/mbtreestats.hpp).
#include "mbtreestats.hpp"
#include <stdlib.h>
#include <string.h>

// The device entries are resolved weakly: a device library without them (an older build; the tests' CPU stand-in) still loads, and the unit moves floats
// and converts them here with the same arithmetic.
#pragma weak x264gpu_mbtree_pack
#pragma weak x264gpu_mbtree_unpack

namespace x264host {

// x264: (int16_t)(offset * 256.0f), byte-swapped.  The C cast truncates toward zero and is undefined out of range; x264's SIMD versions saturate: the rule here
// (NaN -> 0).  The unit is compiled without contraction; both factors are powers of two anyway
uint16_t mbtree_fix8_pack(float offset)
{
    const float v = offset * 256.0f;
    int i;
    if (!(v == v)) i = 0;
    else if (v >= 32767.0f) i = 32767;
    else if (v <= -32768.0f) i = -32768;
    else i = (int)v;
    const unsigned u = (unsigned)i & 0xffffu;
    return (uint16_t)((u >> 8) | ((u & 0xffu) << 8));
}
float mbtree_fix8_unpack(uint16_t word)
{
    const int16_t i = (int16_t)(uint16_t)((word >> 8) | ((word & 0xffu) << 8));
    return (float)i * (1.0f / 256.0f);
}

bool MbTreeStats::opted_in()
{
    const char *e = getenv("X264GPU_MBTREE_STATS");
    return e && atoi(e) == 1;
}

// x264's SLICE_TYPE_* of a picture type / of a statistics character
static int slice_type_of(int pic_type) { return pic_type == PIC_P ? 0 : pic_type == PIC_BREF || pic_type == PIC_B ? 1 : 2; }

bool MbTreeStats::check_read(const x264_param_t &p, const char *stat_in, int nmb_)
{
    nmb = nmb_;
    rank.clear();
    FILE *f = stat_in ? fopen(stat_in, "rb") : nullptr;
    if (!f) return false;          // (the rate control says so and fails the open)
    char line[2048];
    bool header_tree = false, header_seen = false, size_ok = true;
    std::vector<std::pair<int, char>> ent;          // out, type
    while (fgets(line, sizeof(line), f)) {
        if (line[0] == '#') {
            if (!header_seen && !strncmp(line, "#options:", 9)) {
                header_seen = true;
                int w = 0, h = 0;
                if (sscanf(line + 9, " %dx%d", &w, &h) == 2) size_ok = w == p.i_width && h == p.i_height;
                header_tree = strstr(line, " mbtree=1") != nullptr;
            }
            continue;
        }
        int in = 0, out = 0; char t = 0;
        if (sscanf(line, " in:%d out:%d type:%c", &in, &out, &t) == 3) ent.push_back({ out, t });
    }
    fclose(f);
    if (!header_tree) { xlog(&p, X264_LOG_WARNING, "2-pass: the statistics' header lacks mbtree=1 (the first pass ran without the macroblock-tree statistics file): mbtree 0\n"); return false; }
    if (!size_ok) { xlog(&p, X264_LOG_WARNING, "2-pass: resolution changed since the first pass (the statistics' header names another width x height; macroblock-tree offsets are not rescaled in the MI355X path): mbtree 0\n"); return false; }
    // a kept picture's record is the k-th one, k = the kept pictures coded before it
    rank.assign(ent.size(), -1);
    std::vector<char> by_out(ent.size(), 'b');
    for (const auto &e : ent) if (e.first >= 0 && e.first < (int)ent.size()) by_out[(size_t)e.first] = e.second;
    int kept = 0;
    for (size_t k = 0; k < by_out.size(); k++) if (by_out[k] != 'b') rank[k] = kept++;
    path = std::string(stat_in) + ".mbtree";
    FILE *t = fopen(path.c_str(), "rb");
    if (!t) { xlog(&p, X264_LOG_WARNING, "2-pass: the macroblock-tree statistics file is missing (<stats>.mbtree cannot be opened): mbtree 0\n"); rank.clear(); return false; }
    fseek(t, 0, SEEK_END);
    const long have = ftell(t), need = (long)kept * (1 + 2 * (long)nmb);
    fclose(t);
    if (have < need) { xlog(&p, X264_LOG_WARNING, "2-pass: the macroblock-tree statistics file is truncated (%ld bytes, %d kept pictures of %d macroblocks need %ld): mbtree 0\n", have, kept, nmb, need); rank.clear(); return false; }
    return true;
}

bool MbTreeStats::open(const x264_param_t &p, const char *stat_in, const char *stat_out, int nmb_)
{
    if (!writing && !reading) return true;
    nmb = nmb_;
    on_device = x264gpu_mbtree_pack && x264gpu_mbtree_unpack;
    words.assign((size_t)nmb, 0);
    if (on_device) { if (x264gpu_malloc((void **)&d_words, (size_t)nmb * sizeof(uint16_t)) != X264GPU_OK) { xlog(&p, X264_LOG_ERROR, "macroblock-tree statistics: %s\n", x264gpu_last_error()); return false; } }
    else floats.assign((size_t)nmb, 0.f);
    if (writing) {
        path = std::string(stat_out) + ".mbtree";
        file = fopen((path + ".temp").c_str(), "wb");
    } else file = fopen(path.c_str(), "rb");          // (check_read left the name)
    if (!file) { xlog(&p, X264_LOG_ERROR, "ratecontrol_init: can't open mbtree stats file\n"); return false; }
    if (writing && on_device) xlog(&p, X264_LOG_INFO, "2-pass: the macroblock-tree's offsets of every kept picture go to the macroblock-tree statistics file, packed on the device\n");
    else if (writing) xlog(&p, X264_LOG_INFO, "2-pass: the macroblock-tree's offsets of every kept picture go to the macroblock-tree statistics file, packed on the host\n");
    else if (on_device) xlog(&p, X264_LOG_INFO, "2-pass: kept pictures take their quantiser offsets from the macroblock-tree statistics file, unpacked on the device (rc-lookahead 0; other B pictures: AQ alone)\n");
    else xlog(&p, X264_LOG_INFO, "2-pass: kept pictures take their quantiser offsets from the macroblock-tree statistics file, unpacked on the host (rc-lookahead 0; other B pictures: AQ alone)\n");
    return true;
}

bool MbTreeStats::write_record(const x264_param_t &p, int pic_type, const float *d_offsets, void *stream)
{
    if (!writing || !file || !d_offsets) return true;
    bool ok;
    if (on_device) ok = x264gpu_mbtree_pack(d_offsets, nmb, d_words, stream) == X264GPU_OK && x264gpu_memcpy_d2h(words.data(), d_words, words.size() * sizeof(uint16_t), stream) == X264GPU_OK;
    else {
        ok = x264gpu_memcpy_d2h(floats.data(), d_offsets, floats.size() * sizeof(float), stream) == X264GPU_OK;
        for (size_t i = 0; i < floats.size() && ok; i++) words[i] = mbtree_fix8_pack(floats[i]);
    }
    if (!ok) { xlog(&p, X264_LOG_ERROR, "macroblock-tree statistics: %s\n", x264gpu_last_error()); return false; }
    const uint8_t t = (uint8_t)slice_type_of(pic_type);
    if (fwrite(&t, 1, 1, file) != 1 || fwrite(words.data(), sizeof(uint16_t), words.size(), file) != words.size()) {
        xlog(&p, X264_LOG_ERROR, "ratecontrol_end: stats file could not be written to\n");
        return false;
    }
    return true;
}

int MbTreeStats::read_record(const x264_param_t &p, long coded_index, int pic_type, float *d_offsets, void *stream)
{
    if (!reading || !file) return 0;
    if (coded_index < 0 || coded_index >= (long)rank.size() || rank[(size_t)coded_index] < 0 || pic_type == PIC_B) return 0;
    uint8_t t = 0;
    if (fseek(file, (long)rank[(size_t)coded_index] * (1 + 2 * (long)nmb), SEEK_SET) || fread(&t, 1, 1, file) != 1 ||
        fread(words.data(), sizeof(uint16_t), words.size(), file) != words.size()) {
        xlog(&p, X264_LOG_ERROR, "Incomplete MB-tree stats file.\n");
        return -1;
    }
    if (t != slice_type_of(pic_type)) { xlog(&p, X264_LOG_ERROR, "MB-tree frametype %d doesn't match actual frametype %d.\n", (int)t, slice_type_of(pic_type)); return -1; }
    bool ok;
    if (on_device) ok = x264gpu_memcpy_h2d(d_words, words.data(), words.size() * sizeof(uint16_t), stream) == X264GPU_OK && x264gpu_mbtree_unpack(d_words, nmb, d_offsets, stream) == X264GPU_OK;
    else {
        for (size_t i = 0; i < words.size(); i++) floats[i] = mbtree_fix8_unpack(words[i]);
        ok = x264gpu_memcpy_h2d(d_offsets, floats.data(), floats.size() * sizeof(float), stream) == X264GPU_OK;
    }
    if (!ok) { xlog(&p, X264_LOG_ERROR, "macroblock-tree statistics: %s\n", x264gpu_last_error()); return -1; }
    return 1;
}

void MbTreeStats::close(const x264_param_t &p)
{
    const bool opened = file != nullptr;
    if (file) fclose(file);
    file = nullptr;
    if (writing && opened && rename((path + ".temp").c_str(), path.c_str()))
        xlog(&p, X264_LOG_ERROR, "failed to rename \"%s.temp\" to \"%s\"\n", path.c_str(), path.c_str());
    if (d_words) x264gpu_free(d_words);
    d_words = nullptr; writing = reading = false;
}

}  // namespace x264host

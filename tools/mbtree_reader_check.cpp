// mbtree_reader_check.cpp — host/mbtreestats.cpp's file reader fed the tree file cut at every length (and with trailing bytes), a statistics file with damaged
// lines, picture indices outside the statistics and a record of another type.  A stand-alone program for a sanitizer build on the CPU, over the tests' stand-in
// device library (make -C tests/stub):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -Iinclude -Ix264vfw_amd/host tools/mbtree_reader_check.cpp \
//       x264vfw_amd/host/mbtreestats.cpp -Ltests/stub/_build -lx264gpu -Wl,-rpath,$PWD/tests/stub/_build -o /tmp/mbtree_reader_check && /tmp/mbtree_reader_check /tmp
// exit status 0: every short file was refused, every whole one read; the sanitizers report on their own.
#include "mbtreestats.hpp"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
using namespace x264host;
void x264host::xlog(const x264_param_t *p, int level, const char *fmt, ...) { va_list ap; va_start(ap, fmt); fprintf(stderr, "[%d] ", level); vfprintf(stderr, fmt, ap); va_end(ap); }
int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: mbtree_reader_check DIR\n"); return 1; }
    x264_param_t p = {}; p.i_width = 64; p.i_height = 48;
    const int nmb = 12;
    const std::string st = std::string(argv[1]) + "/mbtree_reader_check.stats";
    FILE *f = fopen(st.c_str(), "wb");
    fprintf(f, "#options: 64x48 fps=25/1 rc=crf mbtree=1 rc_lookahead=8\n");
    const char types[] = "IPBbbPiB";
    for (int i = 0; i < 8; i++) fprintf(f, "in:%d out:%d type:%c dur:1 cpbdur:1 q:20.00 aq:20.00 tex:1 mv:1 misc:1 imb:1 pmb:1 smb:1 d:- ref:;\n", i, i, types[i]);
    fprintf(f, "in:99999 out:-7 type:P\n garbage line\n");
    fclose(f);
    const int kept = 6, rs = 1 + 2 * nmb;
    std::string full;
    const int tb[6] = { 2, 0, 1, 0, 2, 1 };
    for (int k = 0; k < kept; k++) { full.push_back((char)tb[k]); for (int i = 0; i < 2 * nmb; i++) full.push_back((char)(k * 31 + i)); }
    int usable = 0, refused = 0;
    for (size_t len = 0; len <= full.size() + 3; len++) {
        f = fopen((st + ".mbtree").c_str(), "wb");
        std::string s = full + "xyz";
        fwrite(s.data(), 1, len, f); fclose(f);
        MbTreeStats t; t.reading = true;
        if (!t.check_read(p, st.c_str(), nmb)) { refused++; t.reading = false; continue; }
        usable++;
        if (!t.open(p, st.c_str(), st.c_str(), nmb)) return 2;
        float *d = nullptr; x264gpu_malloc((void **)&d, nmb * sizeof(float));
        const int kind[8] = { PIC_IDR, PIC_P, PIC_BREF, PIC_B, PIC_B, PIC_P, PIC_I, PIC_BREF };
        for (long c = -2; c < 12; c++) { const int r = t.read_record(p, c, c >= 0 && c < 8 ? kind[c] : PIC_P, d, nullptr); if (c >= 0 && c < 8 && kind[c] != PIC_B && r != 1) return 3; if ((c < 0 || c >= 8) && r != 0) return 4; }
        if (t.read_record(p, 1, PIC_BREF, d, nullptr) != -1) return 5;          // a record of another type
        x264gpu_free(d);
        t.close(p);
    }
    printf("usable %d refused %d (of %zu lengths)\n", usable, refused, full.size() + 4);
    return usable == 4 && refused == (int)full.size() ? 0 : 6;
}

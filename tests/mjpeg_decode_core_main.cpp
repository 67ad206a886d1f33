// Runs the entropy decoder of csrc/mjpeg_decode_core.h - the text the device kernel runs - on the host, so that a build with
// -fsanitize=address,undefined checks its bounds logic over corrupt streams before any of them is given to a GPU
// (tests/test_mjpeg_decode_core_host.py writes the case files and compares what this prints with the Python twin).
//
// A case file, little-endian ints: magic 'MJDC', components, hs, vs, mw, mh, comp_off[3], comp_bw[3], frame_blocks, n_intervals,
// scan_bytes; then one MjdTables record, n_intervals x 4 ints (byte offset, byte length, first MCU, MCU count) and the scan.
// The scan and the coefficients live in exactly sized heap blocks: one byte read or written outside them is a sanitizer report.
// Output per case: "<file> <status>" on stdout, and the coefficients to <file>.coef.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mjpeg_decode_core.h"

static bool read_exact(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        int32_t head[16];
        MjdTables* tables = static_cast<MjdTables*>(malloc(sizeof(MjdTables)));
        if (!read_exact(f, head, sizeof(head)) || head[0] != 0x43444a4d || !read_exact(f, tables, sizeof(MjdTables))) {
            fprintf(stderr, "%s: bad case file\n", argv[a]);
            return 2;
        }
        MjdGeom g;
        g.components = head[1], g.hs = head[2], g.vs = head[3], g.mw = head[4], g.mh = head[5];
        for (int c = 0; c < 3; ++c) g.comp_off[c] = head[6 + c], g.comp_bw[c] = head[9 + c];
        g.frame_blocks = head[12];
        const int n_intervals = head[13], scan_bytes = head[14];
        if (n_intervals < 0 || scan_bytes < 0 || g.frame_blocks < 1 || g.frame_blocks > (1 << 20)) {
            fprintf(stderr, "%s: bad sizes\n", argv[a]);
            return 2;
        }
        std::vector<int32_t> iv((size_t)n_intervals * 4);
        uint8_t* scan = static_cast<uint8_t*>(malloc(scan_bytes ? scan_bytes : 1));
        int16_t* coef = static_cast<int16_t*>(calloc((size_t)g.frame_blocks * 64, sizeof(int16_t)));
        if (!read_exact(f, iv.data(), iv.size() * 4) || !read_exact(f, scan, scan_bytes)) {
            fprintf(stderr, "%s: truncated case file\n", argv[a]);
            return 2;
        }
        fclose(f);
        int status = 0;
        for (int i = 0; i < n_intervals; ++i) {
            const int32_t* v = &iv[(size_t)i * 4];
            // what the C entry point checks before it launches: the bytes inside the scan
            if (v[0] < 0 || v[1] < 0 || (long long)v[0] + v[1] > scan_bytes) {
                fprintf(stderr, "%s: interval %d outside the scan\n", argv[a], i);
                return 2;
            }
            // each interval's bytes in a block of their own: the decoder may not even read its neighbour's
            uint8_t* own = static_cast<uint8_t*>(malloc(v[1] ? v[1] : 1));
            memcpy(own, scan + v[0], v[1]);
            const int st = mjd_decode_interval(own, v[1], v[2], v[3], g, *tables, coef);
            free(own);
            if (st > status) status = st;
        }
        char name[4096];
        snprintf(name, sizeof(name), "%s.coef", argv[a]);
        FILE* o = fopen(name, "wb");
        if (!o || fwrite(coef, 128, g.frame_blocks, o) != (size_t)g.frame_blocks) {
            fprintf(stderr, "cannot write %s\n", name);
            return 2;
        }
        fclose(o);
        printf("%s %d\n", argv[a], status);
        free(coef), free(scan), free(tables);
    }
    return 0;
}

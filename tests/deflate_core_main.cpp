// csrc/deflate_core.h on the host, for tests/test_deflate_core_host.py: built with -fsanitize=address,undefined and run over files of
// histograms. Each argument is a file of little-endian uint32 [k][286] counts, limit 15 bits - or, when its name ends in ".cl", of
// [k][19] counts of the code-length code, limit 7 bits; for each the program writes <file>.out: per histogram its length bytes, then
// its uint16 codes. Without arguments it only proves that it runs. It ends by printing the length-symbol table (length, symbol, extra
// bit count, extra value for 3..258) and the header's order of the code-length symbols, which the test compares with the twin's.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "deflate_core.h"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        const std::string name(argv[a]);
        const bool cl = name.size() > 3 && name.compare(name.size() - 3, 3, ".cl") == 0;
        const size_t nsym = cl ? DFL_NCL : DFL_NSYM;
        const int max_bits = cl ? DFL_CL_MAX_BITS : DFL_MAX_BITS;
        std::vector<uint32_t> counts;
        uint32_t buf[DFL_NSYM];
        while (fread(buf, sizeof(uint32_t), nsym, f) == nsym) counts.insert(counts.end(), buf, buf + nsym);
        fclose(f);
        const std::string out_path = std::string(argv[a]) + ".out";
        FILE* o = fopen(out_path.c_str(), "wb");
        if (!o) return 2;
        for (size_t h = 0; h < counts.size() / nsym; ++h) {
            // exact-size heap blocks: the sanitizer sees a write one element past any of them
            std::vector<uint32_t> count(counts.begin() + h * nsym, counts.begin() + (h + 1) * nsym);
            std::vector<uint8_t> len(nsym);
            std::vector<uint16_t> code(nsym);
            DflScratch* sc = new DflScratch;
            dfl_build_lengths(count.data(), (int)nsym, max_bits, len.data(), sc);
            dfl_codes(len.data(), (int)nsym, code.data(), sc);
            delete sc;
            fwrite(len.data(), 1, nsym, o);
            fwrite(code.data(), 2, nsym, o);
        }
        fclose(o);
    }
    for (int length = 3; length <= 258; ++length) {
        uint32_t extra = 0;
        const uint32_t s = dfl_length_symbol(length, &extra);
        printf("%d %u %u %u\n", length, s & 0xffffu, s >> 16, extra);
    }
    for (int k = 0; k < DFL_NCL; ++k) printf("cl %d %d\n", k, dfl_cl_order(k));
    return 0;
}

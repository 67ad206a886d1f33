// csrc/weight_table.h on the host, for tests/test_weight_table_host.py: built with -fsanitize=address,undefined. Arguments: embed_dim
// depth num_heads features out_channels[0..3] num_frames use_clstoken use_bn pe_rope. It prints, per row of the table,
//   spec <name> <shape ...>
// and, where the row is packed,
//   pack <kind> <key> <name> <N> <K> <npad> <kpad> <row> <packed elements of the key>
// with the true sizes N x K as csrc/host.hip reads them from the shape (a vector is one row). Without arguments it only proves that it runs.
#include <stdio.h>
#include <stdlib.h>

#include "weight_table.h"

int main(int argc, char** argv) {
    if (argc == 1) return 0;
    if (argc != 13) {
        fprintf(stderr, "expected 12 integers, got %d\n", argc - 1);
        return 2;
    }
    int v[12];
    for (int i = 0; i < 12; ++i) v[i] = atoi(argv[i + 1]);
    vda_config c = {};
    c.embed_dim = v[0], c.depth = v[1], c.num_heads = v[2], c.features = v[3];
    for (int i = 0; i < 4; ++i) c.out_channels[i] = v[4 + i];
    c.num_frames = v[8], c.use_clstoken = v[9], c.use_bn = v[10], c.pe_rope = v[11];
    static const char* const kinds[] = {"none", "vec", "mat", "rows", "conv3", "convt", "convt_bias", "geglu", "geglu_bias"};
    const WeightTable table(c);
    printf("pads %d %d %d %d %d\n", table.ocp[0], table.ocp[1], table.ocp[2], table.ocp[3], table.Fhp);
    for (const WEntry& e : table.rows) {
        printf("spec %s", e.name.c_str());
        for (int64_t d : e.shape) printf(" %lld", (long long)d);
        printf("\n");
        if (e.kind != W_NONE)
            printf("pack %s %s %s %d %d %d %d %d %zu\n", kinds[e.kind], e.key.c_str(), e.name.c_str(), e.N(), e.K(), e.npad, e.kpad, e.row, e.packed_elems());
    }
    return 0;
}

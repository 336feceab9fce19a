// tri_records_check.cpp -- ptina_amd/csrc/tri_records.h (the triangle records every builder writes) run by a stand-alone host
// program, so that the numpy restatement of tests/record_checks.py can be held to the header's own words without a GPU:
//
//     c++ -std=c++17 -O2 -ffp-contract=off tools/tri_records_check.cpp -o tri_records_check && ./tri_records_check model.bin records.bin
//
// model.bin:   int32 n, then verts [3n][8] f32 (pos3 nrm3 uv2), then material ids [n] int32
// records.bin: tgeo [n][4][4] f32, tfast [n][3][4] f32, tshade [n][4][4] f32, one triangle after the other in the model's order
// (-ffp-contract=off says for every host compiler what the header's pragma says for clang)

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../ptina_amd/csrc/tri_records.h"

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s model.bin records.bin\n", argv[0]); return 2; }
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 1; }
    int32_t n = 0;
    if (std::fread(&n, sizeof n, 1, in) != 1 || n < 0 || n > (1 << 24)) { std::fprintf(stderr, "%s: no face count\n", argv[1]); return 1; }
    std::vector<float> verts((size_t)n * 24);
    std::vector<int32_t> mtl((size_t)n);
    if (std::fread(verts.data(), sizeof(float), verts.size(), in) != verts.size() || std::fread(mtl.data(), sizeof(int32_t), mtl.size(), in) != mtl.size()) {
        std::fprintf(stderr, "%s: shorter than %d faces\n", argv[1], n);
        return 1;
    }
    std::fclose(in);
    std::vector<MptVec4> tgeo((size_t)n * 4), tfast((size_t)n * 3), tshade((size_t)n * 4);
    for (int f = 0; f < n; f++) {
        const float *p0 = verts.data() + (size_t)f * 24, *p1 = p0 + 8, *p2 = p0 + 16;
        float bits;
        std::memcpy(&bits, &mtl[f], sizeof bits);
        tri_make_tgeo(p0, p1, p2, &tgeo[(size_t)f * 4]);
        tri_make_tfast(&tgeo[(size_t)f * 4], &tfast[(size_t)f * 3]);
        tri_make_tshade(p0, p1, p2, bits, &tshade[(size_t)f * 4]);
    }
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 1; }
    bool ok = true;
    for (const std::vector<MptVec4> *a : { &tgeo, &tfast, &tshade })
        ok = ok && std::fwrite(a->data(), sizeof(MptVec4), a->size(), out) == a->size();
    ok = std::fclose(out) == 0 && ok;
    if (!ok) { std::fprintf(stderr, "%s: write failed\n", argv[2]); return 1; }
    std::printf("tri_records_check: %d triangles\n", n);
    return EXIT_SUCCESS;
}

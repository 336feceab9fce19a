// tree_rules_check.cpp -- the host passes of mpt_build_tree (ptina_amd/csrc/tree_host.h on the rules of tree_rules.h: the LBVH,
// its SAH re-partition, the record packing, the 4-wide collapse) run by a stand-alone host program, so that their bytes can be
// held to recorded ones and to the device passes' without a GPU, and so that they can run under the host sanitizers without
// loading anything into an interpreter:
//
//     c++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread tools/tree_rules_check.cpp -o tree_rules_check
//     ./tree_rules_check model.bin out.bin
//
// (-fsanitize=thread in place of address,undefined for the threads of SahBuild: they start above 16 384 leaves in a range.)
// model.bin: int32 n, positions [n][3][3] f32, int32 tree (1: the fast build walks the SAH tree, 0: the LBVH), int32 sah_exact_max
// out.bin:   int32 {n, ni, depth, fast_depth, nw, wide_depth, wide_stack_levels, 0} with ni = max(n - 1, 0) internal nodes and
//            nw wide nodes, then child [ni][2] i32, leaf [n] i32, mc [n] i32, bmin [ni][3] f32, bmax [ni][3] f32,
//            snode [ni][2][4], fnode [ni][4][4], wnode [nw][8][4], qnode [nw][4][4] (32-bit words)
// (-ffp-contract=off says for every host compiler what the header's pragma says for clang)

#include <cstdio>
#include <cstdlib>
#include "../ptina_amd/csrc/tree_host.h"

template <class T> static bool put(FILE *out, const T *p, size_t count) { return count == 0 || std::fwrite(p, sizeof(T), count, out) == count; }

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s model.bin out.bin\n", argv[0]); return 2; }
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 1; }
    int32_t n = 0, opt[2] = { 1, 8192 };
    if (std::fread(&n, sizeof n, 1, in) != 1 || n < 0 || n > (1 << 24)) { std::fprintf(stderr, "%s: no face count\n", argv[1]); return 1; }
    std::vector<float> pos((size_t)n * 9);
    if (std::fread(pos.data(), sizeof(float), pos.size(), in) != pos.size() || std::fread(opt, sizeof(int32_t), 2, in) != 2) {
        std::fprintf(stderr, "%s: shorter than %d faces and two options\n", argv[1], n);
        return 1;
    }
    std::fclose(in);
    std::vector<float> verts((size_t)n * 24, 0.f);                              // [3n][8] = pos3 nrm3 uv2
    for (size_t v = 0; v < (size_t)n * 3; v++)
        for (int a = 0; a < 3; a++) verts[v * 8 + a] = pos[v * 3 + a];

    const int ni = n > 1 ? n - 1 : 0;
    HostLbvh t;
    if (const char *why = host_lbvh(verts.data(), n, t)) { std::fprintf(stderr, "tree_rules_check: %s\n", why); return 1; }
    std::vector<MptVec4> snode, fnode;
    pack_snode(t, n, snode);
    int fast_depth = t.depth;
    if (opt[0] == 1 && ni > 0) {
        SahBuild sb;
        sb.run(verts.data(), t.leaf.data(), n, opt[1]);
        fast_depth = sb.depth;
        pack_fnode(verts.data(), t.leaf.data(), n, sb.child, sb.blo, sb.bhi, fnode);
    } else {
        pack_fnode(verts.data(), t.leaf.data(), n, lbvh_fast_ids(t, n), t.bmin, t.bmax, fnode);
    }
    HostWide w;
    host_collapse(fnode.data(), n, w);
    const int levels = w.nodes ? wide_stack_levels(w.wnode.data() + WNODE_ID_ROW, 8, (size_t)w.nodes, n) : 0;

    FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 1; }
    const int32_t head[8] = { n, ni, t.depth, fast_depth, w.nodes, w.depth, levels, 0 };
    bool ok = put(out, head, 8);
    ok = ok && put(out, t.child.data(), (size_t)ni * 2) && put(out, t.leaf.data(), (size_t)n) && put(out, t.mc.data(), (size_t)n);
    ok = ok && put(out, t.bmin.data(), (size_t)ni * 3) && put(out, t.bmax.data(), (size_t)ni * 3);
    ok = ok && put(out, snode.data(), (size_t)ni * 2) && put(out, fnode.data(), (size_t)ni * 4);
    ok = ok && put(out, w.wnode.data(), (size_t)w.nodes * 8) && put(out, w.qnode.data(), (size_t)w.nodes * 4);
    ok = std::fclose(out) == 0 && ok;
    if (!ok) { std::fprintf(stderr, "%s: write failed\n", argv[2]); return 1; }
    std::printf("tree_rules_check: %d triangles, depth %d / %d, %d wide nodes\n", n, t.depth, fast_depth, w.nodes);
    return EXIT_SUCCESS;
}

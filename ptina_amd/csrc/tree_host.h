// tree_host.h -- the host passes of mpt_build_tree as functions over plain arrays: the reference LBVH, its SAH re-partition
// for the fast build, the record packing and the 4-wide collapse.  Plain C++17 on the rules of tree_rules.h, with nothing of
// HIP and no context: tree_build.cpp calls them between its downloads and uploads, and the stand-alone program
// tools/tree_rules_check.cpp runs them without a GPU, under the host sanitizers.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>
#include "tree_rules.h"

// ------------------------------------------------------------------ LBVH build (tree/lbvh.py:169-305)
// Same algorithm as the reference (30-bit Morton codes of centroids, sorted, Karras hierarchy,
// bottom-up boxes) with two robustness changes: the sort key is (code << 32 | index), so equal
// codes cannot corrupt the hierarchy, and the boxes are fitted in one post-order
// pass instead of <=64 level-synchronous launches with a read-back each (lbvh.py:251-261).
// With distinct codes the tree is node-for-node the reference's.
struct HostLbvh {
    std::vector<int32_t> child, leaf, mc;      // [n-1][2]: a leaf slot (< n) or an internal node + n; [n] slot -> face; [n] codes
    std::vector<float> bmin, bmax;             // [n-1][3]
    int depth = 0;                             // internal nodes on the longest way down
};

// verts: [3n][8].  -> null, or why there is no tree
inline const char *host_lbvh(const float *verts, int n, HostLbvh &t) {
    // genMortonCodes, lbvh.py:169-183
    float bmin[3] = { 1e6f, 1e6f, 1e6f }, bmax[3] = { -1e6f, -1e6f, -1e6f };
    std::vector<float> cen((size_t)n * 3);
    for (int f = 0; f < n; f++)
        for (int a = 0; a < 3; a++) {
            const float ctr = centroid(verts, f, a);
            cen[(size_t)f * 3 + a] = ctr;
            bmin[a] = fminf(bmin[a], ctr);
            bmax[a] = fmaxf(bmax[a], ctr);
        }
    std::vector<unsigned long long> key(n);
    for (int f = 0; f < n; f++) key[f] = morton_key(&cen[(size_t)f * 3], bmin, bmax, f);
    std::sort(key.begin(), key.end());                                          // lbvh.py:204-208

    t.leaf.resize(n); t.mc.resize(n);
    for (int i = 0; i < n; i++) { t.leaf[i] = (int32_t)(key[i] & 0xffffffffu); t.mc[i] = (int32_t)(key[i] >> 32); }

    const int ni = n > 1 ? n - 1 : 0;
    t.child.assign((size_t)std::max(ni, 1) * 2, 0);
    t.bmin.assign((size_t)std::max(ni, 1) * 3, 0.f);
    t.bmax.assign((size_t)std::max(ni, 1) * 3, 0.f);
    t.depth = 0;
    for (int i = 0; i < ni; i++) lbvh_children(key.data(), n, i, &t.child[(size_t)i * 2], &t.child[(size_t)i * 2 + 1]);
    if (ni == 0) return nullptr;

    // boxes: iterative post-order from the root (also yields the depth the LDS stack must hold)
    static const char *const corrupted = "AABB step never stop! hierarchy corrupted?";      // lbvh.py:259
    std::vector<int> order; order.reserve(ni);
    std::vector<std::pair<int, int>> st; st.push_back({ 0, 1 });
    std::vector<char> seen(ni, 0);
    while (!st.empty()) {
        auto [i, dpt] = st.back(); st.pop_back();
        if (i < 0 || i >= ni || seen[i]) return corrupted;
        seen[i] = 1;
        order.push_back(i);
        t.depth = std::max(t.depth, dpt);
        for (int k = 0; k < 2; k++) {
            int ch = t.child[(size_t)i * 2 + k];
            if (ch >= n) st.push_back({ ch - n, dpt + 1 });
        }
    }
    if ((int)order.size() != ni) return corrupted;
    for (int s = ni - 1; s >= 0; s--) {                                         // children before parents
        int i = order[s];
        float lo[2][3], hi[2][3];
        for (int k = 0; k < 2; k++) {
            int ch = t.child[(size_t)i * 2 + k];
            if (ch < n) leaf_box(verts, t.leaf[ch], lo[k], hi[k]);
            else for (int a = 0; a < 3; a++) { lo[k][a] = t.bmin[(size_t)(ch - n) * 3 + a]; hi[k][a] = t.bmax[(size_t)(ch - n) * 3 + a]; }
        }
        for (int a = 0; a < 3; a++) {
            t.bmin[(size_t)i * 3 + a] = fminf(lo[0][a], lo[1][a]);
            t.bmax[(size_t)i * 3 + a] = fmaxf(hi[0][a], hi[1][a]);
        }
    }
    return nullptr;
}

// ------------------------------------------------------------------ SAH re-partition (fast build only)
// The image does not depend on the tree's shape (only on which of two equal-depth hits wins), so the
// production traversal is free to walk a better tree over the SAME leaf slots: measured on the
// 978-triangle benchmark scene a full-sweep SAH partition needs 11.0 node fetches per ray where the
// LBVH needs 23.7.  Leaves stay single triangles (the node record is unchanged); nodes are numbered
// in DFS pre-order, root 0.  Exact sweep for ranges <= 8192 leaves, 32-bin SAH above.
struct SahBuild {
    int n = 0;
    std::vector<float> lo, hi, ctr;            // per leaf slot [n][3]
    std::vector<int> idx;                      // leaf slots, partitioned in place
    std::vector<int32_t> child;                // [n-1][2]: >= 0 internal, ~slot leaf
    std::vector<float> blo, bhi;               // per internal node [n-1][3]: its own box
    int depth = 0;
    int exact_max = 8192;                      // ranges up to this many leaves: every split of every axis (exact sweep); above: 32 bins

    int split(int b, int e) {                  // returns m in (b, e): [b, m) | [m, e)
        const int cnt = e - b;
        float best = INFINITY;
        int best_axis = -1, best_k = -1;
        float best_pos = 0.f;
        bool binned = cnt > exact_max;
        std::vector<std::pair<float, int>> key(binned ? 0 : cnt);
        std::vector<float> rarea(binned ? 0 : cnt);
        float cl[3] = { INFINITY, INFINITY, INFINITY }, ch[3] = { -INFINITY, -INFINITY, -INFINITY };
        for (int t = b; t < e; t++)
            for (int a = 0; a < 3; a++) {
                cl[a] = std::min(cl[a], ctr[(size_t)idx[t] * 3 + a]);
                ch[a] = std::max(ch[a], ctr[(size_t)idx[t] * 3 + a]);
            }
        for (int a = 0; a < 3; a++) {
            if (!(ch[a] > cl[a])) continue;
            if (!binned) {
                for (int t = 0; t < cnt; t++) key[t] = { ctr[(size_t)idx[b + t] * 3 + a], idx[b + t] };
                std::sort(key.begin(), key.end());
                float l[3] = { INFINITY, INFINITY, INFINITY }, h[3] = { -INFINITY, -INFINITY, -INFINITY };
                for (int t = cnt - 1; t > 0; t--) {
                    int s = key[t].second;
                    for (int q = 0; q < 3; q++) { l[q] = std::min(l[q], lo[(size_t)s * 3 + q]); h[q] = std::max(h[q], hi[(size_t)s * 3 + q]); }
                    rarea[t] = half_area(l, h);
                }
                for (int q = 0; q < 3; q++) { l[q] = INFINITY; h[q] = -INFINITY; }
                for (int k = 1; k < cnt; k++) {
                    int s = key[k - 1].second;
                    for (int q = 0; q < 3; q++) { l[q] = std::min(l[q], lo[(size_t)s * 3 + q]); h[q] = std::max(h[q], hi[(size_t)s * 3 + q]); }
                    float cost = half_area(l, h) * k + rarea[k] * (cnt - k);
                    if (cost < best) { best = cost; best_axis = a; best_k = k; }
                }
            } else {
                const int NB = 32;
                float bl[NB][3], bh[NB][3];
                int bc[NB];
                for (int q = 0; q < NB; q++) { bc[q] = 0; for (int r = 0; r < 3; r++) { bl[q][r] = INFINITY; bh[q][r] = -INFINITY; } }
                float scale = NB / (ch[a] - cl[a]);
                for (int t = b; t < e; t++) {
                    int s = idx[t];
                    int q = std::min(NB - 1, std::max(0, (int)((ctr[(size_t)s * 3 + a] - cl[a]) * scale)));
                    bc[q]++;
                    for (int r = 0; r < 3; r++) { bl[q][r] = std::min(bl[q][r], lo[(size_t)s * 3 + r]); bh[q][r] = std::max(bh[q][r], hi[(size_t)s * 3 + r]); }
                }
                float ra[NB]; int rc[NB];
                float l[3] = { INFINITY, INFINITY, INFINITY }, h[3] = { -INFINITY, -INFINITY, -INFINITY };
                int c2 = 0;
                for (int q = NB - 1; q > 0; q--) {
                    c2 += bc[q];
                    for (int r = 0; r < 3; r++) { l[r] = std::min(l[r], bl[q][r]); h[r] = std::max(h[r], bh[q][r]); }
                    ra[q] = half_area(l, h); rc[q] = c2;
                }
                for (int r = 0; r < 3; r++) { l[r] = INFINITY; h[r] = -INFINITY; }
                int c1 = 0;
                for (int q = 1; q < NB; q++) {
                    c1 += bc[q - 1];
                    for (int r = 0; r < 3; r++) { l[r] = std::min(l[r], bl[q - 1][r]); h[r] = std::max(h[r], bh[q - 1][r]); }
                    if (c1 == 0 || rc[q] == 0) continue;
                    float cost = half_area(l, h) * c1 + ra[q] * rc[q];
                    if (cost < best) { best = cost; best_axis = a; best_k = c1; best_pos = cl[a] + q / scale; }
                }
            }
        }
        if (best_axis < 0) return b + cnt / 2;                 // all centroids equal: split the range in half
        if (!binned) {
            for (int t = 0; t < cnt; t++) key[t] = { ctr[(size_t)idx[b + t] * 3 + best_axis], idx[b + t] };
            std::sort(key.begin(), key.end());
            for (int t = 0; t < cnt; t++) idx[b + t] = key[t].second;
            return b + best_k;
        }
        int a = best_axis;
        const int NB = 32;
        float scale = NB / (ch[a] - cl[a]);
        int qsplit = (int)std::lround((best_pos - cl[a]) * scale);
        int m = (int)(std::partition(idx.begin() + b, idx.begin() + e, [&](int s) {
                          int q = std::min(NB - 1, std::max(0, (int)((ctr[(size_t)s * 3 + a] - cl[a]) * scale)));
                          return q < qsplit;
                      }) - idx.begin());
        if (m <= b || m >= e) m = b + cnt / 2;
        return m;
    }

    std::atomic<int> adepth{0};

    // A range [b, e) of k leaf slots becomes a subtree of exactly k - 1 internal nodes, so in DFS pre-order the
    // node of the range is `me`, its left subtree starts at me + 1 and its right subtree at me + (m - b): the
    // numbering needs no shared counter, subtrees touch disjoint parts of idx / child / blo / bhi, and the big
    // ones are built by threads of their own (1 M leaves: 1.5 s on one core).  The result does not depend on
    // how the work was split.
    void build_range(int b, int e, int me, int dep, int spawn_levels) {
        for (;;) {
            int d0 = adepth.load(std::memory_order_relaxed);
            while (dep > d0 && !adepth.compare_exchange_weak(d0, dep, std::memory_order_relaxed)) {}
            float l[3] = { INFINITY, INFINITY, INFINITY }, h[3] = { -INFINITY, -INFINITY, -INFINITY };
            for (int t = b; t < e; t++)
                for (int q = 0; q < 3; q++) { l[q] = std::min(l[q], lo[(size_t)idx[t] * 3 + q]); h[q] = std::max(h[q], hi[(size_t)idx[t] * 3 + q]); }
            for (int q = 0; q < 3; q++) { blo[(size_t)me * 3 + q] = l[q]; bhi[(size_t)me * 3 + q] = h[q]; }
            const int m = split(b, e);
            const int left = me + 1, right = me + (m - b);
            if (m - b == 1) child[(size_t)me * 2 + 0] = ~idx[b]; else child[(size_t)me * 2 + 0] = left;
            if (e - m == 1) child[(size_t)me * 2 + 1] = ~idx[m]; else child[(size_t)me * 2 + 1] = right;
            const bool has_l = m - b > 1, has_r = e - m > 1;
            if (has_l && has_r) {
                if (spawn_levels > 0 && std::max(m - b, e - m) > 16384) {
                    // (a lopsided split keeps its spawn levels for the big half; a thread that cannot be created -- pid /
                    // ulimit limits in a container -- must not take the process down: the half is built here instead)
                    bool spawned = false;
                    std::thread th;
                    if (std::min(m - b, e - m) > 4096) {
                        try { th = std::thread([=] { build_range(b, m, left, dep + 1, spawn_levels - 1); }); spawned = true; }
                        catch (const std::system_error &) { spawned = false; }
                    }
                    if (!spawned) build_range(b, m, left, dep + 1, spawn_levels - 1);
                    build_range(m, e, right, dep + 1, spawn_levels - 1);
                    if (spawned) th.join();
                    return;
                }
                build_range(b, m, left, dep + 1, 0);          // the smaller worlds recurse; depth is bounded by the tree's
                b = m; me = right; dep += 1; spawn_levels = 0;
            } else if (has_l) { e = m; me = left; dep += 1; }
            else if (has_r) { b = m; me = right; dep += 1; }
            else return;
        }
    }

    void run() {
        const int ni = n > 1 ? n - 1 : 0;
        child.assign((size_t)std::max(ni, 1) * 2, 0);
        blo.assign((size_t)std::max(ni, 1) * 3, 0.f);
        bhi.assign((size_t)std::max(ni, 1) * 3, 0.f);
        idx.resize(n);
        for (int i = 0; i < n; i++) idx[i] = i;
        depth = 0;
        if (ni == 0) return;
        adepth.store(0);
        build_range(0, n, 0, 1, 5);                            // up to 2^5 subtrees in flight
        depth = adepth.load();
    }

    // the re-partition of the faces_n leaves in the order of leaf (slot -> face): exact sweeps up to sah_exact_max leaves
    void run(const float *verts, const int32_t *leaf, int faces_n, int sah_exact_max) {
        n = faces_n;
        exact_max = sah_exact_max;
        lo.resize((size_t)n * 3); hi.resize((size_t)n * 3); ctr.resize((size_t)n * 3);
        for (int slot = 0; slot < n; slot++) {
            float *l = &lo[(size_t)slot * 3], *h = &hi[(size_t)slot * 3];
            leaf_box(verts, leaf[slot], l, h);
            for (int a = 0; a < 3; a++) ctr[(size_t)slot * 3 + a] = 0.5f * (l[a] + h[a]);
        }
        run();
    }
};

// ------------------------------------------------------------------ records
// snode records from the LBVH: {bmin, child0} {bmax, child1}
inline void pack_snode(const HostLbvh &t, int n, std::vector<MptVec4> &snode) {
    const int ni = n > 1 ? n - 1 : 0;
    snode.assign((size_t)std::max(ni, 1) * 2, MptVec4{ 0, 0, 0, 0 });
    for (int i = 0; i < ni; i++) {
        const float *lo = &t.bmin[(size_t)i * 3], *hi = &t.bmax[(size_t)i * 3];
        snode[(size_t)i * 2 + 0] = { lo[0], lo[1], lo[2], asf(t.child[(size_t)i * 2]) };
        snode[(size_t)i * 2 + 1] = { hi[0], hi[1], hi[2], asf(t.child[(size_t)i * 2 + 1]) };
    }
}

// the LBVH's child ids as the fast build names them (its node boxes are bmin / bmax as they are)
inline std::vector<int32_t> lbvh_fast_ids(const HostLbvh &t, int n) {
    std::vector<int32_t> ids(t.child.size());
    for (size_t k = 0; k < ids.size(); k++) ids[k] = lbvh_fast_id(t.child[k], n);
    return ids;
}

// fnode records for the fast build from a (child, box) description over leaf slots: child ids >= 0 internal, ~slot leaf; a node
// record holds its two children's boxes
inline void pack_fnode(const float *verts, const int32_t *leaf, int n, const std::vector<int32_t> &fchild, const std::vector<float> &flo,
                       const std::vector<float> &fhi, std::vector<MptVec4> &fnode) {
    const int ni = n > 1 ? n - 1 : 0;
    fnode.assign((size_t)std::max(ni, 1) * 4, MptVec4{ 0, 0, 0, 0 });
    for (int i = 0; i < ni; i++)
        for (int k = 0; k < 2; k++) {
            const int id = fchild[(size_t)i * 2 + k];
            float l[3], h[3];
            if (id < 0) leaf_box(verts, leaf[~id], l, h);
            else for (int a = 0; a < 3; a++) { l[a] = flo[(size_t)id * 3 + a]; h[a] = fhi[(size_t)id * 3 + a]; }
            fnode_write_child(fnode.data(), i * 2 + k, l, h, id);
        }
}

// ------------------------------------------------------------------ the 4-wide collapse
// The binary tree the fast build walks (fnode: a node record holds its two children's boxes), collapsed into 4-wide nodes for
// the gather kernel, breadth first: wb_grow, wb_exact_record and wb_quantise per node (tree_rules.h).  A ray then makes about
// half as many dependent record fetches, which is what the scenes that do not fit LDS wait for.
struct HostWide {
    std::vector<MptVec4> wnode, qnode;         // [nodes][8], [nodes][4]
    int nodes = 0, depth = 0;
    // expected dependent fetches per ray ~ sum of the surface areas of the nodes that are fetched (SAH argument):
    // over all internal nodes for the binary tree, over the nodes wide records are grown from for the collapse
    double area_bin = 0.0, area_wide = 0.0;
};

inline void host_collapse(const MptVec4 *fnode, int n, HostWide &out) {
    out = HostWide{};
    const int ni = n > 1 ? n - 1 : 0;
    if (ni < 1) return;
    std::vector<float> node_area((size_t)ni, 0.f);
    {
        WbChild two[2];
        wb_children_of(fnode, 0, two);
        node_area[0] = wb_own_area(two);
        for (int b = 0; b < ni; b++) {
            wb_children_of(fnode, b, two);
            for (int k = 0; k < 2; k++) if (two[k].id >= 0) node_area[two[k].id] = wb_area(two[k]);
        }
    }
    for (int b = 0; b < ni; b++) out.area_bin += node_area[b];
    out.wnode.reserve((size_t)ni * 4);
    out.qnode.reserve((size_t)ni * 2);
    std::vector<int> bin_of;            // wide node -> the binary node it was grown from
    std::vector<int> depth_of;
    bin_of.push_back(0); depth_of.push_back(1);
    out.depth = 1;
    for (size_t w = 0; w < bin_of.size(); w++) {
        WbChild ch[4];
        wb_children_of(fnode, bin_of[w], ch);
        out.area_wide += node_area[bin_of[w]];
        const int cnt = wb_grow(fnode, ch);
        int ids[4];
        MptVec4 rec[8], q[4];
        wb_exact_record(ch, cnt, ~n, ids, rec);
        for (int k = 0; k < cnt; k++)
            if (ids[k] >= 0) {                  // an internal child: the next wide node
                bin_of.push_back(ids[k]);
                ids[k] = (int)bin_of.size() - 1;
                depth_of.push_back(depth_of[w] + 1);
                out.depth = std::max(out.depth, depth_of[w] + 1);
            }
        rec[WNODE_ID_ROW] = wb_id_row(ids);
        wb_quantise(ch, cnt, ids, q);
        out.wnode.insert(out.wnode.end(), rec, rec + 8);
        out.qnode.insert(out.qnode.end(), q, q + 4);
    }
    out.nodes = (int)bin_of.size();
}

// The stack levels a traversal of the 4-wide tree can ask for, exactly (render_kernel_lds4 keeps them all in LDS): a step at a
// node with k children leaves up to k - 1 entries behind and goes on with one child; children come after their parents in the
// array.  ids: the id vector of node w at ids[w * stride]; an unused slot names leaf n
inline int wide_stack_levels(const MptVec4 *ids, size_t stride, size_t nw, int n) {
    std::vector<int> need(nw, 0);
    for (size_t w = nw; w-- > 0;) {
        const MptVec4 &idv = ids[w * stride];
        const int32_t id[4] = { asi(idv.x), asi(idv.y), asi(idv.z), asi(idv.w) };
        int k = 0, deep = 0;
        for (int q = 0; q < 4; q++) {
            if (id[q] != ~n) k++;
            if (id[q] >= 0 && (size_t)id[q] < nw) deep = std::max(deep, need[id[q]]);
        }
        need[w] = std::max(k - 1, 0) + deep;
    }
    return 1 + (nw ? need[0] : 0) + 1;      // the sentinel below, and the level the step's last (unwanted) plain store lands on
}

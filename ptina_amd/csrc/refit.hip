// refit.hip -- the boxes of the trees the fast build walks, fitted again to a model whose faces moved (mpt_refit_tree).
//
// The topology is the last build's: the id rows of fnode (binary, SAH or LBVH -- the same kernel fits either) and of wnode /
// qnode (the 4-wide collapse) stay as they are, and every box is recomputed bottom-up from the vertices.
//   link   once per build (the build drops the cache): neither record stores parents, so one lane per node writes, for every
//          internal child, the slot of the parent's record its box lives in: 2 * node + k (fnode), 4 * node + k (wnode); the
//          root gets -1
//   fit    one lane per node.  A node whose children are all leaves starts a climb.  The climbing lane holds a finished node:
//          it takes the boxes of the node's leaf children from the vertices (min / max of the triangle's three vertices,
//          tree_rules.h leaf_box) and those of its internal children from the node's own record, where the lanes that
//          finished them put them; writes the leaf children's boxes (and, for a wide node, the quantised record: tree_rules.h,
//          the collapse's arithmetic); stores the union into its slot of the parent's record; and takes a ticket on the parent's
//          arrival word.  The lane whose ticket is the parent's last internal child goes on with the parent, every other lane
//          ends.  No lane ever waits for another: there is no spin and no poll, so the kernel ends whatever the scheduling.
//          The hand-over is fit_boxes_kernel's (lbvh_build.hip): every word that crosses lanes is written and read with
//          agent-scope atomic accesses, the stores are drained (s_waitcnt vmcnt(0)) before the ticket, and the loads depend on
//          the ticket.  Only fminf / fmaxf touch a box, and a node's union is formed by one lane in slot order, so the bytes do
//          not depend on who arrives when.
//   cost   the sum over every child box of every fnode record of area(child) / area(root) -- the boxes a random ray is
//          expected to meet (SAH) -- in units of 2^-40 as integers (tree_rules.h), so the same bits in any order
// Compiled with -ffp-contract=off like the builders: the bytes are specified (tests/refit_ref.py).

#include <hip/hip_runtime.h>
#include <algorithm>
#include "mpt_types.h"
#include "tree_rules.h"      // the leaf box, the records' layouts, the quantisation and the fixed-point area: the builders' own

#define RF_BLOCK 256

__device__ __forceinline__ float rf_load(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rf_store(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------ links
// width 2: fnode (4 float4 per node, ids in row 3 .xy; an internal child's id is >= 0 -- the root, node 0, is nobody's child);
// width 4: wnode (8 float4 per node, ids in row 6; an internal child's id is in 1 .. count - 1, an unused slot names a leaf)
template <int WIDTH>
__global__ __launch_bounds__(RF_BLOCK) void rf_link_kernel(const MptVec4 *__restrict__ rec, int count, int *__restrict__ parent_slot) {
    const int i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= count) return;
    const MptVec4 idv = rec[(size_t)i * (2 * WIDTH) + (WIDTH == 2 ? FNODE_ID_ROW : WNODE_ID_ROW)];
    const int ids[4] = { asi(idv.x), asi(idv.y), asi(idv.z), asi(idv.w) };
#pragma unroll
    for (int k = 0; k < WIDTH; k++)
        if (ids[k] > 0 && ids[k] < count) parent_slot[ids[k]] = WIDTH * i + k;
    if (i == 0) parent_slot[0] = -1;
}

// ------------------------------------------------------------------ the binary records
// fnode record: rows a = 0..2 {lo0[a], lo1[a], hi0[a], hi1[a]}, row 3 {id0, id1, -, -}; an id < 0 names leaf slot ~id
__global__ __launch_bounds__(RF_BLOCK) void rf_fit_bin_kernel(const float *__restrict__ verts, const int *__restrict__ leaf,
                                                              MptVec4 *fnode, const int *__restrict__ parent_slot, int ni,
                                                              unsigned *arrive) {
    const int i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= ni) return;
    int node = i;
    int id[2];
    {
        const float *rec = (const float *)(fnode + (size_t)node * 4);
        id[0] = asi(rec[fnode_id(0)]); id[1] = asi(rec[fnode_id(1)]);
    }
    if (id[0] >= 0 || id[1] >= 0) return;                       // an internal child: whoever finishes the last of them goes on here
    for (;;) {
        float *rec = (float *)(fnode + (size_t)node * 4);
        float lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            float l[3], h[3];
            if (id[k] < 0) {
                leaf_box(verts, leaf[~id[k]], l, h);
#pragma unroll
                for (int a = 0; a < 3; a++) { rec[fnode_lo(k, a)] = l[a]; rec[fnode_hi(k, a)] = h[a]; }     // (read by later launches only)
            } else {
#pragma unroll
                for (int a = 0; a < 3; a++) { l[a] = rf_load(rec + fnode_lo(k, a)); h[a] = rf_load(rec + fnode_hi(k, a)); }
            }
#pragma unroll
            for (int a = 0; a < 3; a++) { lo[a] = k ? fminf(lo[a], l[a]) : l[a]; hi[a] = k ? fmaxf(hi[a], h[a]) : h[a]; }
        }
        const int ps = parent_slot[node];
        if (ps < 0) break;                                      // the root
        const int p = ps >> 1, k = ps & 1;
        float *prec = (float *)(fnode + (size_t)p * 4);
        id[0] = asi(prec[fnode_id(0)]); id[1] = asi(prec[fnode_id(1)]);     // (the id row is never written here)
#pragma unroll
        for (int a = 0; a < 3; a++) { rf_store(prec + fnode_lo(k, a), lo[a]); rf_store(prec + fnode_hi(k, a), hi[a]); }
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the box is out before the arrival is counted
        const unsigned prev = __hip_atomic_fetch_add(arrive + p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev + 1u != (unsigned)((id[0] >= 0) + (id[1] >= 0))) break;   // a sibling is still on its way: it will finish p
        __asm__ volatile("" ::: "memory");
        node = p;
    }
}

// ------------------------------------------------------------------ the 4-wide records
// wnode record: rows {lo.x[4]} {hi.x[4]} {lo.y[4]} {hi.y[4]} {lo.z[4]} {hi.z[4]} {id[4]} {-}; the used slots come first, an unused
// slot holds empty_id (= ~n) and keeps its 1e30 boxes; qnode is rewritten from the node's exact child boxes by wb_quantise
__global__ __launch_bounds__(RF_BLOCK) void rf_fit_wide_kernel(const float *__restrict__ verts, const int *__restrict__ leaf,
                                                               MptVec4 *wnode, MptVec4 *qnode, const int *__restrict__ parent_slot,
                                                               int nw, int empty_id, unsigned *arrive) {
    const int i = blockIdx.x * RF_BLOCK + threadIdx.x;
    if (i >= nw) return;
    int node = i;
    int id[4];
    {
        const float *rec = (const float *)(wnode + (size_t)node * 8);
#pragma unroll
        for (int k = 0; k < 4; k++) id[k] = asi(rec[wnode_id(k)]);
    }
    if (id[0] > 0 || id[1] > 0 || id[2] > 0 || id[3] > 0) return;
    for (;;) {
        float *rec = (float *)(wnode + (size_t)node * 8);
        WbChild ch[4];
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            ch[k].id = id[k];
            if (id[k] == empty_id) continue;
            cnt = k + 1;
            if (id[k] < 0) {
                leaf_box(verts, leaf[~id[k]], ch[k].lo, ch[k].hi);
#pragma unroll
                for (int a = 0; a < 3; a++) { rec[wnode_lo(k, a)] = ch[k].lo[a]; rec[wnode_hi(k, a)] = ch[k].hi[a]; }
            } else {
#pragma unroll
                for (int a = 0; a < 3; a++) { ch[k].lo[a] = rf_load(rec + wnode_lo(k, a)); ch[k].hi[a] = rf_load(rec + wnode_hi(k, a)); }
            }
        }
        wb_quantise(ch, cnt, id, qnode + (size_t)node * 4);
        const int ps = parent_slot[node];
        if (ps < 0) break;                                      // the root
        float lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = ch[0].lo[a]; hi[a] = ch[0].hi[a]; }
        for (int k = 1; k < cnt; k++)
#pragma unroll
            for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], ch[k].lo[a]); hi[a] = fmaxf(hi[a], ch[k].hi[a]); }
        const int p = ps >> 2, k = ps & 3;
        float *prec = (float *)(wnode + (size_t)p * 8);
        int nint = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) { id[q] = asi(prec[wnode_id(q)]); nint += id[q] > 0; }
#pragma unroll
        for (int a = 0; a < 3; a++) { rf_store(prec + wnode_lo(k, a), lo[a]); rf_store(prec + wnode_hi(k, a), hi[a]); }
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned prev = __hip_atomic_fetch_add(arrive + p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev + 1u != (unsigned)nint) break;
        __asm__ volatile("" ::: "memory");
        node = p;
    }
}

// ------------------------------------------------------------------ cost
// (at most 512 workgroups stride over the nodes, one atomic each: wb_area_kernel's shape)
__global__ __launch_bounds__(RF_BLOCK) void rf_cost_kernel(const MptVec4 *__restrict__ fnode, int ni, unsigned long long *__restrict__ sum) {
    __shared__ unsigned long long wtot[RF_BLOCK / 64];
    const double ra = wb_root_area(fnode);
    unsigned long long a = 0ull;
    for (int b = blockIdx.x * RF_BLOCK + threadIdx.x; b < ni; b += gridDim.x * RF_BLOCK) {
        WbChild ch[2];
        wb_children_of(fnode, b, ch);
        a += wb_fixed_share(wb_area(ch[0]), ra) + wb_fixed_share(wb_area(ch[1]), ra);
    }
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off);
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0ull;
        for (int w = 0; w < RF_BLOCK / 64; w++) t += wtot[w];
        if (t) atomicAdd(sum, t);
    }
}

// ------------------------------------------------------------------ launchers
static inline int rf_grid(int count) { return (count + RF_BLOCK - 1) / RF_BLOCK; }

// parent slots of the ni binary nodes into bin_parent [ni] and of the nw wide nodes into wide_parent [nw] (nw = 0: no wide tree)
MPT_KERNEL_API hipError_t mpt_refit_link(const MptVec4 *fnode, int ni, const MptVec4 *wnode, int nw, int *bin_parent, int *wide_parent,
                                         hipStream_t stream) {
    if (ni > 0) hipLaunchKernelGGL(rf_link_kernel<2>, dim3(rf_grid(ni)), dim3(RF_BLOCK), 0, stream, fnode, ni, bin_parent);
    if (nw > 0) hipLaunchKernelGGL(rf_link_kernel<4>, dim3(rf_grid(nw)), dim3(RF_BLOCK), 0, stream, wnode, nw, wide_parent);
    return hipGetLastError();
}

// *sum += the cost of the binary records (the caller zeroes it)
MPT_KERNEL_API hipError_t mpt_refit_cost(const MptVec4 *fnode, int ni, unsigned long long *sum, hipStream_t stream) {
    if (ni > 0) hipLaunchKernelGGL(rf_cost_kernel, dim3(std::min(rf_grid(ni), 512)), dim3(RF_BLOCK), 0, stream, fnode, ni, sum);
    return hipGetLastError();
}

// fits fnode [ni] and, with nw > 0, wnode / qnode [nw] to verts; arrive: max(ni, nw) words, zeroed here before each pass
MPT_KERNEL_API hipError_t mpt_refit_fit(const float *verts, const int *leaf, int n, MptVec4 *fnode, const int *bin_parent, MptVec4 *wnode,
                                        MptVec4 *qnode, int nw, const int *wide_parent, unsigned *arrive, hipStream_t stream) {
    const int ni = n > 1 ? n - 1 : 0;
    hipError_t e;
    if (ni < 1) return hipSuccess;
    if ((e = hipMemsetAsync(arrive, 0, (size_t)ni * sizeof(unsigned), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(rf_fit_bin_kernel, dim3(rf_grid(ni)), dim3(RF_BLOCK), 0, stream, verts, leaf, fnode, bin_parent, ni, arrive);
    if (nw > 0) {
        if ((e = hipMemsetAsync(arrive, 0, (size_t)nw * sizeof(unsigned), stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(rf_fit_wide_kernel, dim3(rf_grid(nw)), dim3(RF_BLOCK), 0, stream, verts, leaf, wnode, qnode, wide_parent, nw, ~n,
                           arrive);
    }
    return hipGetLastError();
}

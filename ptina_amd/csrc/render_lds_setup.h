// render_lds_setup.h -- how an LDS-resident kernel gets its scene into LDS and is launched: the copy-in of the node records with
// their id rewriting, of the triangles and materials behind them, the walks' regions, and the launch that takes a CU's whole
// dynamic LDS.  Stated once for the two render kernels (render_kernel.hip) and the test door through the walks (walk_eval.hip),
// which must set a walk up exactly as its render kernel does.  Production build only; included behind render_lane.h.
#pragma once
#include <atomic>

// What both walks hold besides their node records, from the kernel's regions: the triangles, the material records and bytes; and the
// lane's column of the int16 stack region
template <class WALK>
DEV void lds_walk_regions(WALK &w, typename WALK::Lifo &stk, MptVec4 *smem, const MptLdsRegions &lay) {
    const int nnode4 = lay.nnode4, ntri4 = lay.ntri4, nmat4 = lay.nmat4, nmtl4 = lay.nmtl4;
    w.tgeo = (LdsVec4Ptr)(void *)(smem + nnode4);
    w.mats = (LdsVec4Ptr)(void *)(smem + nnode4 + ntri4);
    w.mtl = (LdsU8Ptr)(void *)(smem + nnode4 + ntri4 + nmat4);
    stk.stack = (LdsShortPtr)(void *)(smem + nnode4 + ntri4 + nmat4 + nmtl4) + threadIdx.x;
    stk.sp = 0;
}

// The copy-in both kernels make behind their node records: the triangles, the material records (DEFAULT_LAST: the records the model
// uses, then the default one) and one material-record byte per triangle (no_mtl: the byte of a triangle without a material)
template <bool DEFAULT_LAST>
DEV void lds_copy_tris_mats(const MptRenderParams &p, MptVec4 *smem, const MptLdsRegions &lay, int no_mtl) {
    const int nnode4 = lay.nnode4, ntri4 = lay.ntri4, nmat4 = lay.nmat4;
    for (int k = threadIdx.x; k < ntri4; k += blockDim.x) smem[nnode4 + k] = p.tfast[k];
    for (int k = threadIdx.x; k < nmat4; k += blockDim.x) {
        const int rec = k / MPT_LDS_MAT_VEC4, w = k - rec * MPT_LDS_MAT_VEC4;
        const int grec = DEFAULT_LAST && rec == p.lds_nmats ? p.default_mtl : rec;
        smem[nnode4 + ntri4 + k] = ((const MptVec4 *)(p.mats + grec))[w < 4 ? w : w + 4];
    }
    unsigned char *mtl = (unsigned char *)(smem + nnode4 + ntri4 + nmat4);
    for (int k = threadIdx.x; k < p.n; k += blockDim.x) {
        const int id = __float_as_int(p.tshade[(size_t)k * 4 + 3].w);
        mtl[k] = (unsigned char)(id == -1 ? no_mtl : id);
    }
}

// The binary node records (p.fnode) into LDS, MPT_LDS_NODE_STRIDE bytes apart; the ids LdsWalk reads
DEV void lds_copy_nodes(const MptRenderParams &p, MptVec4 *smem) {
    for (int k = threadIdx.x; k < (p.n - 1) * 4; k += blockDim.x) {          // 8-byte stores: the records are 8-byte aligned
        MptVec4 v = p.fnode[k];
        if ((k & 3) == 3) {                        // {id0, id1, -, -}: internal ids become byte offset / 8
            const int i0 = __float_as_int(v.x), i1 = __float_as_int(v.y);
            v.x = __int_as_float(i0 >= 0 ? i0 * (MPT_LDS_NODE_STRIDE / 8) : i0);
            v.y = __int_as_float(i1 >= 0 ? i1 * (MPT_LDS_NODE_STRIDE / 8) : i1);
        }
        float *d = (float *)((char *)smem + (k >> 2) * MPT_LDS_NODE_STRIDE + (k & 3) * 16);
        *(float2 *)d = make_float2(v.x, v.y); *(float2 *)(d + 2) = make_float2(v.z, v.w);
    }
}

// The first seven float4 of every 4-wide node record (p.wnode) into LDS; the ids LdsWalk4 reads
DEV void lds_copy_nodes4(const MptRenderParams &p, MptVec4 *smem) {
    for (int k = threadIdx.x; k < p.nwide * 7; k += blockDim.x) {
        const int rec = k / 7, w = k - rec * 7;
        MptVec4 v = p.wnode[rec * 8 + w];
        if (w == 6) {
            // the four ids (LdsWalk4::ODD_IDS): internal ones become the record's byte offset, leaves (slot << 4) | 1
            const int i0 = __float_as_int(v.x), i1 = __float_as_int(v.y), i2 = __float_as_int(v.z), i3 = __float_as_int(v.w);
#define MPT_LDS_ID(i) __int_as_float((i) >= 0 ? (i) * MPT_LDS4_NODE_STRIDE : ((~(i)) << 4) | 1)
            v.x = MPT_LDS_ID(i0); v.y = MPT_LDS_ID(i1); v.z = MPT_LDS_ID(i2); v.w = MPT_LDS_ID(i3);
#undef MPT_LDS_ID
        }
        smem[k] = v;
    }
}

// LdsWalk4's node ids are LDS addresses counted from 0: the dynamic LDS must be all the LDS its kernel has (it is; a static
// __shared__ object added to it one day would move smem)
DEV bool lds_starts_at_zero(MptVec4 *smem) { return (unsigned)(unsigned long long)(LdsBytePtr)(LdsVec4Ptr)(void *)smem == 0u; }

// a kernel that takes the whole dynamic LDS of a CU (lds_layout.h): lds_bytes = scene records + 2 KiB per stack level; grid = one
// persistent workgroup per CU.  One instance -- and one "attribute set" flag -- per kernel instantiation.
template <auto KERNEL, class... A>
static hipError_t launch_whole_lds(int grid, int block, size_t lds_bytes, hipStream_t stream, const A &...args) {
    // function attributes are per device: remember which devices have been told about the 160 KiB
    static std::atomic<bool> configured[MPT_MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MPT_MAX_DEVICES) return hipErrorInvalidDevice;
    if (!configured[dev].load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, MPT_LDS_BUDGET);
        if (e != hipSuccess) return e;
        configured[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(block), lds_bytes, stream, args...);
    return hipGetLastError();
}

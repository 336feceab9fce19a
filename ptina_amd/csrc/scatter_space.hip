// scatter_space.hip -- the minimum distance of a spaced scatter on the device (the rule stands in
// scatter_rule.h and include/miptina.h): of M candidates -- the selection kernel's records -- the greedy pass in candidate order
// keeps j iff no kept k < j lies closer than r, and the first `count` kept become the scatter's sticky records.
//
// The greedy pass as rounds.  Every candidate has a state: undecided, kept or rejected.  In a round an undecided j looks at the
// states of its conflicting lower-index neighbours: any kept -> j is rejected; else none undecided -> j is kept; else j waits
// (mpt_scatter_space_decide).  A state only moves from undecided to its final value, and the final value of j is a function of the
// final values of lower candidates alone, so whatever a look sees -- the state a neighbour had before the launch, or the one it
// takes during it -- a decision taken is the greedy one.  The lowest undecided candidate decides in every round, so the rounds
// end; with random priorities a handful do.  A ROUND IS A LAUNCH: no kernel here waits for another workgroup, and kernel boundaries
// are the only synchronisation.  The host launches MPT_SPACE_BATCH rounds, waits, and reads per scatter the last round in which a
// lane of it still waited (a mapped word: the waiting waves store the round's number, one lane each); a scatter that waited in the
// batch's last round gets another batch.  A round in which a lane is decided returns at that lane's first test.
//
// The grid.  Looking at every lower candidate costs M^2 / 2 tests, so a uniform grid over the box of the finite positions finds the
// neighbours: cell edge h, cell c(x) = floor((x - lo) / h) per axis, the cells hashed into a table of 2^k >= M buckets; bucket
// membership by count (integer vector atomics), exclusive scan and fill.  The order inside a bucket is whatever the atomics made it:
// a look is a predicate over the SET of neighbours, so it cannot reach the result.  Two cells that share a bucket only add
// candidates that then fail the distance test, and a bucket reached twice from one lane is looked at twice, to the same end.
// A position with a coordinate that is not finite conflicts with nothing (every comparison with NaN or of inf < inf is false): it
// is kept at once and never enters the grid.
//
// The 27 cells around a candidate's own miss no conflicting pair.  Let j, k conflict: d2 = ((dx dx) + (dy dy)) + (dz dz) < r2 as
// computed.  Rounded sums of non-negative terms are not below their terms, so fl(dx dx) <= d2 < fl(r r), hence |dx| < r (1 + 2^-52),
// and with dx = fl(xj - xk) the true |xj - xk| < r (1 + 2^-51); alike for y and z.
//   * the edge is a hair above r: h >= fl(r (1 + 2^-20)) > r (1 + 2^-21), so |xj - xk| < h (1 - 2^-22);
//   * the edge is clamped from below by 2^-20 of the box's largest extent (mpt_space_edge), so u(x) = fl(fl(x - lo) / h) <= 2^20 + 1
//     for every x of the box: the cell coordinates are integers an int holds exactly, and u carries an error of at most
//     u 2^-52 <= 2^-31.  So u(xj) - u(xk) < (1 - 2^-22) + 2^-30 < 1 for xk <= xj, and cells two or more apart would need a
//     difference above 1: |c(xj) - c(xk)| <= 1;
//   * c is a monotone function of x (x - lo, / h and floor are, under rounding as well), so c(lo) = 0 <= c(x) <= c(hi): a
//     neighbouring cell outside [0, c(hi)] holds nobody and is skipped, and the cell counts n = c(hi) + 1 come from the same function.
// A box whose extent is not finite has one cell, and every pair is tested.
//
// Kernels, one lane per candidate (or per bucket), a workgroup of 256 lanes in ONE scatter (run_table.h), one launch of each kind per
// compose whatever the number of spaced scatters:
//   space_position_kernel   per candidate: its position from its record and the surface as it stands (explicit points: as given);
//                           the workgroup's box of finite positions to part[block]
//   space_fold_kernel       one workgroup per scatter: the box, the edge, the cell counts
//   space_count_kernel      per candidate: undecided and +1 on its bucket, or kept at once (not finite)
//   space_scan_kernel       one workgroup per scatter: the exclusive scan of its buckets' counts, 4096 at a time (16 a lane) with a carry
//   space_fill_kernel       per candidate: its slot in its bucket (+1 on the bucket's cursor)
//   space_round_kernel      per candidate: a round
//   space_compact_kernel    one workgroup per scatter: the scan of the kept flags, 4096 at a time with a carry; the first `count`
//                           kept records into the sticky arena, their candidate indices beside; the number kept to the host's mapped word
// Vector stores and vector atomics only; job and surface row are uniform in a workgroup.

#include <math.h>
#include "scatter_dev.h"

static_assert(sizeof(MptSpaceJob) == 72 && sizeof(MptSpaceGrid) == 48, "the records scatter_space.hip reads and writes");

enum { SPACE_PER = 16 };                    // consecutive items a lane takes in the two kernels that scan with a carry
struct SpaceLane { int r, item, i; };
// the run, the spaced scatter and the candidate of this lane
static __device__ __forceinline__ SpaceLane space_lane(const MptRun *__restrict__ runs, int nruns) {
    SpaceLane l;
    l.r = mpt_run_of(runs, nruns);
    l.item = runs[l.r].item;
    l.i = ((int)blockIdx.x - runs[l.r].block) * SC_BLOCK + (int)threadIdx.x;
    return l;
}

static __device__ __forceinline__ bool space_finite(const double *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// the workgroup's smallest x, to every lane (fmin: exact, order-free; the largest is -min(-x))
static __device__ __forceinline__ double space_block_min(double x, double *s_part) {
#pragma unroll
    for (int d = SC_WAVE / 2; d > 0; d >>= 1) x = fmin(x, __shfl_xor(x, d, SC_WAVE));
    __syncthreads();                           // (s_part was read by the call before)
    if (((int)threadIdx.x & (SC_WAVE - 1)) == 0) s_part[(int)threadIdx.x / SC_WAVE] = x;
    __syncthreads();
    x = s_part[0];
    for (int k = 1; k < SC_WAVES; k++) x = fmin(x, s_part[k]);
    return x;
}

__global__ __launch_bounds__(SC_BLOCK) void space_position_kernel(const float4 *__restrict__ pool, const MptComposeObj *__restrict__ objs,
                                                                  const MptScatterJob *__restrict__ jobs, const MptSpaceJob *__restrict__ sjobs,
                                                                  const MptRun *__restrict__ runs, int nruns, const MptScatterPoint *__restrict__ records,
                                                                  double *__restrict__ pos, double *__restrict__ part) {
    __shared__ double s_part[SC_WAVES];
    const SpaceLane l = space_lane(runs, nruns);
    const MptSpaceJob &s = sjobs[l.item];
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (l.i < s.m) {
        double *p = pos + (s.at + l.i) * 3;
        double P[3];
        if (s.job >= 0) {
            const MptScatterJob &o = jobs[s.job];
            const MptScatterPoint rec = records[s.cand_at + l.i];
            P[0] = P[1] = P[2] = NAN;
            if ((unsigned)rec.face < (unsigned)o.nfaces) {                 // (a guard of the reads: the records are the selection kernel's own)
                double C[3][3];
                sc_corners(pool, objs[o.surf_obj], rec.face, C, nullptr);
                mpt_scatter_point_of(C[0], C[1], C[2], rec, P);
            }
            p[0] = P[0]; p[1] = P[1]; p[2] = P[2];
        } else {
            P[0] = p[0]; P[1] = p[1]; P[2] = p[2];
        }
        if (space_finite(P))
            for (int k = 0; k < 3; k++) { lo[k] = P[k]; hi[k] = P[k]; }
    }
    for (int k = 0; k < 3; k++) {
        const double a = space_block_min(lo[k], s_part), b = -space_block_min(-hi[k], s_part);
        if (threadIdx.x == 0) { part[(size_t)blockIdx.x * 6 + k] = a; part[(size_t)blockIdx.x * 6 + 3 + k] = b; }
    }
}

__global__ __launch_bounds__(SC_BLOCK) void space_fold_kernel(const MptSpaceJob *__restrict__ sjobs, const MptRun *__restrict__ runs, int nruns, int blocks,
                                                              const double *__restrict__ part, MptSpaceGrid *__restrict__ grids) {
    __shared__ double s_part[SC_WAVES];
    const int r = (int)blockIdx.x;
    int b0, b1;
    sc_run_blocks(runs, nruns, blocks, r, &b0, &b1);
    double lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        double a = INFINITY, b = INFINITY;
        for (int q = b0 + (int)threadIdx.x; q < b1; q += SC_BLOCK) { a = fmin(a, part[(size_t)q * 6 + k]); b = fmin(b, -part[(size_t)q * 6 + 3 + k]); }
        lo[k] = space_block_min(a, s_part);
        hi[k] = -space_block_min(b, s_part);
    }
    if (threadIdx.x != 0) return;
    if (!(lo[0] <= hi[0])) { for (int k = 0; k < 3; k++) lo[k] = hi[k] = 0.0; }   // no finite position at all
    const MptSpaceJob &s = sjobs[runs[r].item];
    MptSpaceGrid g;
    g.h = mpt_space_edge(s.r, lo, hi);
    for (int k = 0; k < 3; k++) { g.lo[k] = lo[k]; g.n[k] = mpt_space_cell(hi[k], lo[k], g.h) + 1; }
    g.pad = 0;
    grids[runs[r].item] = g;
}

// the bucket of position p in the table of scatter s
static __device__ __forceinline__ uint32_t space_bucket_of(const MptSpaceGrid &g, const MptSpaceJob &s, const double *p, int c[3]) {
    for (int k = 0; k < 3; k++) c[k] = mpt_space_cell(p[k], g.lo[k], g.h);
    return mpt_space_bucket(c[0], c[1], c[2], s.mask);
}

__global__ __launch_bounds__(SC_BLOCK) void space_count_kernel(const MptSpaceJob *__restrict__ sjobs, const MptSpaceGrid *__restrict__ grids,
                                                               const MptRun *__restrict__ runs, int nruns, const double *__restrict__ pos,
                                                               int32_t *__restrict__ state, uint32_t *__restrict__ cursor) {
    const SpaceLane l = space_lane(runs, nruns);
    const MptSpaceJob &s = sjobs[l.item];
    if (l.i >= s.m) return;
    const double *p = pos + (s.at + l.i) * 3;
    const bool in = space_finite(p);
    state[s.state_at + l.i] = in ? MPT_SPACE_UNDECIDED : MPT_SPACE_KEPT;
    if (!in) return;
    int c[3];
    atomicAdd(cursor + s.bucket_at + space_bucket_of(grids[l.item], s, p, c), 1u);
}

// cursor[bucket] holds the bucket's count: start[bucket] = the exclusive scan, and the cursor begins there
__global__ __launch_bounds__(SC_BLOCK) void space_scan_kernel(const MptSpaceJob *__restrict__ sjobs, const MptRun *__restrict__ runs,
                                                              uint32_t *__restrict__ cursor, uint32_t *__restrict__ start) {
    __shared__ uint64_t s_sum[SC_WAVES];
    const MptSpaceJob &s = sjobs[runs[blockIdx.x].item];
    const int64_t nb = (int64_t)s.mask + 1;
    uint64_t carry = 0;
    for (int64_t base = 0; base < nb; base += SC_BLOCK * SPACE_PER) {
        const int64_t b0 = base + (int64_t)threadIdx.x * SPACE_PER;
        uint32_t x[SPACE_PER];
        uint64_t sum = 0;
#pragma unroll
        for (int k = 0; k < SPACE_PER; k++) { x[k] = b0 + k < nb ? cursor[s.bucket_at + b0 + k] : 0u; sum += x[k]; }
        uint64_t total;
        uint64_t before = carry + sc_block_scan(sum, s_sum, &total);
#pragma unroll
        for (int k = 0; k < SPACE_PER; k++) {
            if (b0 + k < nb) { start[s.bucket_at + b0 + k] = (uint32_t)before; cursor[s.bucket_at + b0 + k] = (uint32_t)before; }
            before += x[k];
        }
        carry += total;
    }
}

__global__ __launch_bounds__(SC_BLOCK) void space_fill_kernel(const MptSpaceJob *__restrict__ sjobs, const MptSpaceGrid *__restrict__ grids,
                                                              const MptRun *__restrict__ runs, int nruns, const double *__restrict__ pos,
                                                              uint32_t *__restrict__ cursor, int32_t *__restrict__ items) {
    const SpaceLane l = space_lane(runs, nruns);
    const MptSpaceJob &s = sjobs[l.item];
    if (l.i >= s.m) return;
    const double *p = pos + (s.at + l.i) * 3;
    if (!space_finite(p)) return;
    int c[3];
    const uint32_t slot = atomicAdd(cursor + s.bucket_at + space_bucket_of(grids[l.item], s, p, c), 1u);
    if (slot < (uint32_t)s.m) items[s.at + slot] = l.i;                    // (below M: the counts' scan; a guard of the store)
}

// round `round` (from 1).  `state` is read and written in place, and is not read through the scalar cache
__global__ __launch_bounds__(SC_BLOCK) void space_round_kernel(const MptSpaceJob *__restrict__ sjobs, const MptSpaceGrid *__restrict__ grids,
                                                               const MptRun *__restrict__ runs, int nruns, const double *__restrict__ pos,
                                                               const uint32_t *__restrict__ start, const uint32_t *__restrict__ cursor,
                                                               const int32_t *__restrict__ items, int32_t *state, uint32_t *left_host, unsigned round) {
    const SpaceLane l = space_lane(runs, nruns);
    const MptSpaceJob &s = sjobs[l.item];
    if (l.i >= s.m || state[s.state_at + l.i] != MPT_SPACE_UNDECIDED) return;
    const MptSpaceGrid &g = grids[l.item];
    const double *base = pos + s.at * 3, *p = base + (size_t)l.i * 3;
    const double me[3] = { p[0], p[1], p[2] };
    int c[3];
    space_bucket_of(g, s, me, c);
    bool any_kept = false, any_undecided = false;
    for (int d = 0; d < 27 && !any_kept; d++) {
        const int x = c[0] + d % 3 - 1, y = c[1] + d / 3 % 3 - 1, z = c[2] + d / 9 - 1;
        if ((unsigned)x >= (unsigned)g.n[0] || (unsigned)y >= (unsigned)g.n[1] || (unsigned)z >= (unsigned)g.n[2]) continue;
        const uint32_t b = mpt_space_bucket(x, y, z, s.mask);
        uint32_t q = start[s.bucket_at + b], end = cursor[s.bucket_at + b];
        if (end > (uint32_t)s.m) end = (uint32_t)s.m;                      // (a guard of the reads)
        for (; q < end && !any_kept; q++) {
            const int k = items[s.at + q];
            if ((unsigned)k >= (unsigned)l.i || !mpt_scatter_conflict(me, base + (size_t)k * 3, s.r2)) continue;
            const int32_t sk = state[s.state_at + k];
            any_kept |= sk == MPT_SPACE_KEPT;
            any_undecided |= sk == MPT_SPACE_UNDECIDED;
        }
    }
    const int mine = mpt_scatter_space_decide(any_kept, any_undecided);
    if (mine != MPT_SPACE_UNDECIDED) { state[s.state_at + l.i] = mine; return; }
    // the lanes that wait: the first of them in the wave tells the host that this scatter needs round + 1
    const unsigned long long waiting = __ballot(1);
    if (((int)threadIdx.x & (SC_WAVE - 1)) == __ffsll((long long)waiting) - 1) left_host[l.item] = round;
}

__global__ __launch_bounds__(SC_BLOCK) void space_compact_kernel(const MptSpaceJob *__restrict__ sjobs, const MptRun *__restrict__ runs,
                                                                 const int32_t *__restrict__ state, const MptScatterPoint *records, MptScatterPoint *points,
                                                                 int32_t *__restrict__ index, uint32_t *__restrict__ kept_host) {
    __shared__ uint64_t s_sum[SC_WAVES];
    const int item = runs[blockIdx.x].item;
    const MptSpaceJob &s = sjobs[item];
    uint64_t carry = 0;
    for (int base = 0; base < s.m; base += SC_BLOCK * SPACE_PER) {
        const int i0 = base + (int)threadIdx.x * SPACE_PER;
        unsigned kept = 0;                     // bit k: candidate i0 + k is kept
#pragma unroll
        for (int k = 0; k < SPACE_PER; k++)
            if (i0 + k < s.m && state[s.state_at + i0 + k] == MPT_SPACE_KEPT) kept |= 1u << k;
        uint64_t total;
        uint64_t rank = carry + sc_block_scan((uint64_t)__popc(kept), s_sum, &total);
        for (int k = 0; k < SPACE_PER && rank < (uint64_t)s.count; k++) {
            if (!(kept >> k & 1u)) continue;
            points[s.point_at + rank] = records[s.cand_at + i0 + k];
            index[s.point_at + rank] = i0 + k;
            rank++;
        }
        carry += total;
    }
    if (threadIdx.x == 0) kept_host[item] = (uint32_t)carry;
}

// ---------------------------------------------------------------- launchers
// runs[nruns] and blocks: the plan over the spaced scatters' candidates (run_table.h; an item is a row of sjobs); part holds 6
// values per block; cursor and start a word per bucket (cursor comes zeroed), state and items a word and pos three values per candidate
MPT_KERNEL_API hipError_t mpt_launch_space_grid(const float *pool, const MptComposeObj *objs, const MptScatterJob *jobs, const MptSpaceJob *sjobs,
                                                const MptRun *runs, int nruns, int blocks, const MptScatterPoint *records, double *pos, double *part,
                                                MptSpaceGrid *grids, int32_t *state, uint32_t *cursor, uint32_t *start, int32_t *items, hipStream_t stream) {
    if (nruns < 1 || blocks < 1) return hipErrorInvalidValue;
    const dim3 all((unsigned)blocks), each((unsigned)nruns), wg(SC_BLOCK);
    hipLaunchKernelGGL(space_position_kernel, all, wg, 0, stream, (const float4 *)pool, objs, jobs, sjobs, runs, nruns, records, pos, part);
    hipLaunchKernelGGL(space_fold_kernel, each, wg, 0, stream, sjobs, runs, nruns, blocks, (const double *)part, grids);
    hipLaunchKernelGGL(space_count_kernel, all, wg, 0, stream, sjobs, (const MptSpaceGrid *)grids, runs, nruns, (const double *)pos, state, cursor);
    hipLaunchKernelGGL(space_scan_kernel, each, wg, 0, stream, sjobs, runs, cursor, start);
    hipLaunchKernelGGL(space_fill_kernel, all, wg, 0, stream, sjobs, (const MptSpaceGrid *)grids, runs, nruns, (const double *)pos, cursor, items);
    return hipGetLastError();
}

// rounds first .. first + n - 1
MPT_KERNEL_API hipError_t mpt_launch_space_rounds(const MptSpaceJob *sjobs, const MptSpaceGrid *grids, const MptRun *runs, int nruns, int blocks,
                                                  const double *pos, const uint32_t *start, const uint32_t *cursor, const int32_t *items, int32_t *state,
                                                  uint32_t *left_host, unsigned first, int n, hipStream_t stream) {
    if (nruns < 1 || blocks < 1 || n < 1) return hipErrorInvalidValue;
    for (int k = 0; k < n; k++)
        hipLaunchKernelGGL(space_round_kernel, dim3((unsigned)blocks), dim3(SC_BLOCK), 0, stream, sjobs, grids, runs, nruns, pos, start, cursor, items, state,
                           left_host, first + (unsigned)k);
    return hipGetLastError();
}

MPT_KERNEL_API hipError_t mpt_launch_space_compact(const MptSpaceJob *sjobs, const MptRun *runs, int nruns, const int32_t *state,
                                                   const MptScatterPoint *records, MptScatterPoint *points, int32_t *index, uint32_t *kept_host,
                                                   hipStream_t stream) {
    if (nruns < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(space_compact_kernel, dim3((unsigned)nruns), dim3(SC_BLOCK), 0, stream, sjobs, runs, state, records, points, index, kept_host);
    return hipGetLastError();
}

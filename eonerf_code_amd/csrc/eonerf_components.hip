// Connected components of a sampled volume under the mesher's own connectivity (include/eonerf_components.h): a union-find in LDS per
// tile, a union over the edges between tiles, a flatten, the counts, and the element-wise filter.  The rule's predicates and the
// refusals are in eonerf_components_check.h; this file is the launches.
// `labels` is the parent array from the first launch on.  Its invariant: an entry of a point on the side is >= 0 and <= its own index,
// and only ever decreases (plain stores of LOCAL, atomicMin of MERGE, the root itself in FLATTEN); every other entry is -1 and stays.
// So every walk towards a root moves to strictly smaller indices and ends, whatever copy of an entry a load returns: a stale parent is
// an older ancestor of the same tree.  The loops below also stop on a value that breaks the invariant rather than follow it.
// Cost: every kernel is memory bound; per point LOCAL reads 4 and writes 8 bytes, MERGE reads 4 on the tile faces, FLATTEN reads 8 and
// writes up to 8, COUNTS reads 4 (8 at roots), the filter reads 8 and writes 4.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/eonerf_components.h"
#include "../../include/eonerf_hip.h"
#include "eonerf_components_check.h"

namespace {

// ---- the walks --------------------------------------------------------------------------------------------------------------------
// Scope::load reads a parent without ever reusing a value a register or this CU's L1 holds; Scope::lower is an atomic minimum.
struct Lds {
    static __device__ inline int load(const int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static __device__ inline int lower(int* a, int v) { return __hip_atomic_fetch_min(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct Agent {
    static __device__ inline int load(const int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ inline int lower(int* a, int v) { return __hip_atomic_fetch_min(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

template <class S>
__device__ inline int cc_find(const int* parent, int x) {
    for (;;) {
        const int y = S::load(parent + x);
        if (y >= x || y < 0) return x;          // y == x: a root.  Anything else here breaks the invariant and ends the walk.
        x = y;
    }
}

// cc_find with path halving: an entry is lowered to its grandparent, read through the entry's own two links, and to nothing else.  So
// only parent[x] changes, to a node x's own chain led to; no walk that starts below x sees a difference, which is what the loop of
// cc_union relies on when it goes on with the pair it displaced.  (Lowering every entry of a walk to the root found at its end would
// NOT be safe: a second walk may pass through a link another union has just put in, and would hang that union's operand below a root
// of the other tree before the union has joined the two.)  A tile face makes hundreds of unions between the same two trees; the walks
// shorten by half each time.
template <class S>
__device__ inline int cc_find_halving(int* parent, int x) {
    for (;;) {
        const int y = S::load(parent + x);
        if (y >= x || y < 0) return x;
        const int z = S::load(parent + y);
        if (z >= y || z < 0) return y;
        S::lower(parent + x, z);
        x = z;
    }
}

// Joins the trees of a and b.  old = the parent hi had: where hi was no root (a stale read, or another thread was faster) its old link
// may just have been replaced by lo, or lo may not have been taken, so the pair (old, lo) is still to be joined; its larger end is
// below hi, so the loop ends.
template <class S, bool kHalving>
__device__ inline void cc_union(int* parent, int a, int b) {
    auto find = [parent](int x) { return kHalving ? cc_find_halving<S>(parent, x) : cc_find<S>(parent, x); };
    a = find(a);
    b = find(b);
    while (a != b) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = S::lower(parent + hi, lo);
        if (old >= hi || old == lo || old < 0) break;
        a = find(old);
        b = find(lo);
    }
}

// ---- LOCAL ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCcBlock) void k_cc_local(const float* f, int nx, int ny, int nz, unsigned tx, unsigned ty, float level, int side,
                                                       int* labels, unsigned* info) {
    __shared__ int par[kCcTile];
    __shared__ unsigned acc[kCcTile];
    const unsigned bx = blockIdx.x % tx, byz = blockIdx.x / tx, by = byz % ty, bz = byz / ty;
    const int tid = threadIdx.x, ix = tid & (kCcTx - 1), jy = tid / kCcTx;       // round r is the tile's layer kz = r
    static_assert(kCcBlock == kCcTx * kCcTy, "one round of the workgroup is one z layer of the tile");
    const int i = (int)bx * kCcTx + ix, j = (int)by * kCcTy + jy, k0 = (int)bz * kCcTz;
    const bool col = i < nx && j < ny;
    unsigned on = 0;
#pragma unroll
    for (int r = 0; r < kCcRounds; ++r) {
        const int l = r * kCcBlock + tid, k = k0 + r;
        bool mine = false;
        if (col && k < nz) mine = cc_on_side(f[((size_t)k * ny + j) * nx + i], level, side);
        par[l] = mine ? l : -1;
        acc[l] = 0u;
        on |= (unsigned)mine << r;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kCcRounds; ++r) {
        if (!((on >> r) & 1)) continue;
        const int l = r * kCcBlock + tid;
        for (int s = 0; s < 7; ++s) {
            const int d = cc_dir(s), dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
            if (ix + dx >= kCcTx || jy + dy >= kCcTy || r + dz >= kCcTz) continue;          // the edge leaves the tile: MERGE's
            const int l2 = l + dx + dy * kCcTx + dz * kCcBlock;
            if (Lds::load(par + l2) >= 0) cc_union<Lds, false>(par, l, l2);                        // the sign of an entry never changes
        }
    }
    __syncthreads();
    int root[kCcRounds];
    const int lane = tid & 63;
#pragma unroll
    for (int r = 0; r < kCcRounds; ++r) {
        const bool mine = (on >> r) & 1;
        root[r] = mine ? cc_find<Lds>(par, r * kCcBlock + tid) : -1;
        const bool edge = mine && cc_on_boundary(i, j, k0 + r, nx, ny, nz);
        // one add per wavefront for the lanes that share the first lane's root (a solid tile: all of them), one per lane for the rest
        const unsigned long long m = __ballot(mine);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        const int r0 = __shfl(root[r], leader, 64);
        const bool same = mine && root[r] == r0;
        const unsigned long long ms = __ballot(same), me = __ballot(same && edge);
        if (lane == leader) {
            atomicAdd(&acc[r0], (unsigned)__popcll(ms));
            if (me) atomicOr(&acc[r0], EONERF_CC_BOUNDARY);
        }
        if (mine && !same) {
            atomicAdd(&acc[root[r]], 1u);
            if (edge) atomicOr(&acc[root[r]], EONERF_CC_BOUNDARY);
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kCcRounds; ++r) {
        const int l = r * kCcBlock + tid, k = k0 + r;
        if (!col || k >= nz) continue;
        const size_t p = ((size_t)k * ny + j) * nx + i;
        int label = -1;
        if (root[r] >= 0) {
            const int rx = root[r] & (kCcTx - 1), ry = (root[r] / kCcTx) & (kCcTy - 1), rz = root[r] / kCcBlock;
            label = (int)((((size_t)k0 + rz) * ny + ((size_t)by * kCcTy + ry)) * nx + ((size_t)bx * kCcTx + rx));
        }
        labels[p] = label;
        info[p] = root[r] == l ? acc[l] : 0u;
    }
}

// ---- MERGE ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCcBlock) void k_cc_merge(int* parent, int nx, int ny, int nz, unsigned n) {
    const unsigned p = blockIdx.x * (unsigned)kCcBlock + threadIdx.x;
    if (p >= n) return;
    const unsigned q = p / (unsigned)nx;
    const int i = (int)(p - q * (unsigned)nx), j = (int)(q % (unsigned)ny), k = (int)(q / (unsigned)ny);
    // the last point of its tile on an axis, with a neighbour beyond it: the forward edges that step on that axis leave the tile
    const bool cx = (i & (kCcTx - 1)) == kCcTx - 1 && i + 1 < nx, cy = (j & (kCcTy - 1)) == kCcTy - 1 && j + 1 < ny,
               cz = (k & (kCcTz - 1)) == kCcTz - 1 && k + 1 < nz;
    if (!(cx || cy || cz)) return;
    if (Agent::load(parent + p) < 0) return;
    const unsigned unx = (unsigned)nx, nxy = (unsigned)nx * (unsigned)ny;
    auto on_side = [parent](unsigned at) { return Agent::load(parent + at) >= 0; };
    for (int s = 0; s < 7; ++s) {
        const int d = cc_dir(s);
        if (!(((d & 1) && cx) || ((d & 2) && cy) || ((d & 4) && cz))) continue;             // stays inside the tile: LOCAL's
        if (((d & 1) && i + 1 >= nx) || ((d & 2) && j + 1 >= ny) || ((d & 4) && k + 1 >= nz)) continue;      // no far end in the lattice
        const unsigned far = p + mesh_corner_offset(d, unx, nxy);
        if (!on_side(far)) continue;
        // Edges that other edges imply are left out: a solid tile face would otherwise make 256 x 7 unions between the same two trees.
        bool implied = false;
        if (d & (d - 1)) {
            // a diagonal p -> p + d, where a point between them is on the side: p + e for a part e of d; the edges e and d - e exist
            // then, both are among the seven directions, and each is joined by its own owner (LOCAL, or this launch)
            for (int e = (d - 1) & d; e && !implied; e = (e - 1) & d) implied = on_side(p + mesh_corner_offset(e, unx, nxy));
        } else {
            // a straight edge whose neighbour one step back along the face (y for an x edge, x for the others) is the same edge between
            // the same two tiles: that one is joined by its owner (or implied in turn, back to the first of the run), and both ends hang
            // together with it inside their tiles
            const bool has_back = d == 1 ? (j & (kCcTy - 1)) != 0 : (i & (kCcTx - 1)) != 0;
            const unsigned back = d == 1 ? unx : 1u;
            implied = has_back && on_side(p - back) && on_side(far - back);
        }
        if (!implied) cc_union<Agent, true>(parent, (int)p, (int)far);
    }
}

// ---- FLATTEN ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCcBlock) void k_cc_flatten(int* labels, unsigned* info, unsigned n) {
    const unsigned p = blockIdx.x * (unsigned)kCcBlock + threadIdx.x;
    if (p >= n) return;
    const int l = Agent::load(labels + p);
    if (l < 0) return;
    const int root = cc_find<Agent>(labels, l);
    // other threads may walk through this entry while it is written: the root is an ancestor like any other
    if (root != l) __hip_atomic_store(labels + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned mine = info[p];                           // not 0: p was its tile's root for this component
    if (mine && root != (int)p) {
        atomicAdd(info + root, mine & ~EONERF_CC_BOUNDARY);
        if (mine & EONERF_CC_BOUNDARY) atomicOr(info + root, EONERF_CC_BOUNDARY);
        info[p] = 0u;
    }
}

// ---- COUNTS -----------------------------------------------------------------------------------------------------------------------
// sum of a and of b over the workgroup, on thread 0
__device__ inline void block_sums(unsigned& a, unsigned& b) {
    __shared__ unsigned part[2][kCcBlock / 64];
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = a; part[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = 0;
        for (int w = 0; w < kCcBlock / 64; ++w) { a += part[0][w]; b += part[1][w]; }
    }
}

// A fixed grid (kCcCountBlocks workgroups at most) strides over the points: three atomics per workgroup, not per 256 points.
__global__ __launch_bounds__(kCcBlock) void k_cc_counts(const int* labels, const unsigned* info, unsigned n, unsigned long long* counts,
                                                        unsigned long long* largest) {
    unsigned roots = 0, points = 0;
    unsigned long long best = 0ull;
    const unsigned stride = gridDim.x * (unsigned)kCcBlock;                 // n <= 2^28 and stride <= 2^19: p + stride does not wrap
    for (unsigned p = blockIdx.x * (unsigned)kCcBlock + threadIdx.x; p < n; p += stride) {
        const int l = labels[p];
        points += l >= 0;
        if (l >= 0 && l == (int)p) {
            ++roots;
            const unsigned long long mine = cc_pack_largest(info[p] & ~EONERF_CC_BOUNDARY, p);
            best = mine > best ? mine : best;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_down(best, o, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(largest, best);
    block_sums(roots, points);
    if (threadIdx.x == 0) {
        if (roots) atomicAdd(counts + 0, (unsigned long long)roots);
        if (points) atomicAdd(counts + 1, (unsigned long long)points);
    }
}

__global__ void k_cc_finish(const unsigned long long* largest, long long* counts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long v = *largest;
        counts[2] = cc_largest_size(v);
        counts[3] = cc_largest_root(v);
    }
}

// ---- the filter -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCcBlock) void k_cc_filter(const float* f, const int* labels, const unsigned* info, unsigned n, int side,
                                                        long long min_points, int protect, float* f_out, unsigned long long* dropped) {
    const unsigned p = blockIdx.x * (unsigned)kCcBlock + threadIdx.x;
    unsigned comps = 0, points = 0;
    if (p < n) {
        const int l = labels[p];
        float v = f[p];
        if (l >= 0 && cc_dropped(info[l], min_points, protect)) {
            v = cc_fill(side);
            points = 1;
            comps = l == (int)p;
        }
        f_out[p] = v;
    }
    block_sums(comps, points);
    if (threadIdx.x == 0) {
        if (comps) atomicAdd(dropped + 0, (unsigned long long)comps);
        if (points) atomicAdd(dropped + 1, (unsigned long long)points);
    }
}

constexpr int kCcCountBlocks = EONERF_CC_COUNT_BLOCKS;                                          // eight workgroups per CU
inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + kCcBlock - 1) / kCcBlock); }     // n <= 2^28: at most 2^20 workgroups

}  // namespace

extern "C" {

int eonerf_cc_version(void) { return EONERF_CC_VERSION; }

size_t eonerf_cc_workspace_bytes(int nx, int ny, int nz) { return cc_workspace_bytes(nx, ny, nz); }

int eonerf_cc_label(const float* f, int nx, int ny, int nz, float level, int side, int32_t* labels, uint32_t* info, int64_t* counts_dev,
                    void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = cc_check_label(f, nx, ny, nz, level, side, labels, info, counts_dev, workspace, workspace_bytes);
    if (rc != EONERF_OK) return rc;
    const unsigned n = (unsigned)mesh_points(nx, ny, nz);
    const CcTiles t = cc_tiles(nx, ny, nz);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts_dev, 0, 4 * sizeof(int64_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(workspace, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return (int)e;
    unsigned long long* largest = (unsigned long long*)workspace;
    hipLaunchKernelGGL(k_cc_local, dim3((unsigned)t.tiles), dim3(kCcBlock), 0, s, f, nx, ny, nz, (unsigned)t.tx, (unsigned)t.ty, level, side,
                       (int*)labels, (unsigned*)info);
    hipLaunchKernelGGL(k_cc_merge, dim3(blocks_of(n)), dim3(kCcBlock), 0, s, (int*)labels, nx, ny, nz, n);
    hipLaunchKernelGGL(k_cc_flatten, dim3(blocks_of(n)), dim3(kCcBlock), 0, s, (int*)labels, (unsigned*)info, n);
    const unsigned count_blocks = blocks_of(n) < (unsigned)kCcCountBlocks ? blocks_of(n) : (unsigned)kCcCountBlocks;
    hipLaunchKernelGGL(k_cc_counts, dim3(count_blocks), dim3(kCcBlock), 0, s, (const int*)labels, (const unsigned*)info, n,
                       (unsigned long long*)counts_dev, largest);
    hipLaunchKernelGGL(k_cc_finish, dim3(1), dim3(64), 0, s, (const unsigned long long*)largest, (long long*)counts_dev);
    return (int)hipGetLastError();
}

int eonerf_cc_filter(const float* f, const int32_t* labels, const uint32_t* info, int nx, int ny, int nz, int side, int64_t min_points,
                     int protect_boundary, float* f_out, int64_t* dropped_dev, void* stream) {
    const int rc = cc_check_filter(f, labels, info, nx, ny, nz, side, min_points, protect_boundary, f_out, dropped_dev);
    if (rc != EONERF_OK) return rc;
    const unsigned n = (unsigned)mesh_points(nx, ny, nz);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(dropped_dev, 0, 2 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_cc_filter, dim3(blocks_of(n)), dim3(kCcBlock), 0, s, f, (const int*)labels, (const unsigned*)info, n, side,
                       (long long)min_points, protect_boundary, f_out, (unsigned long long*)dropped_dev);
    return (int)hipGetLastError();
}

}  // extern "C"

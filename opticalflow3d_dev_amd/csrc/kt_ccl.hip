// kt_ccl.hip — area opening of the reliability mask (of3d_mask_open): MATLAB's
// bwareaopen(rel > relThresh, minSize) of the reference's figure scripts
// (plot_figure4_timeTraces.m:75-79, plot_figure5.m:87-88, plot_figure3_ROIfigures.m:96), per
// ROI box, on the device; of3d_mask_open_pair: the same opening of the joint mask of two
// channels (plot_figure3_ROIfigures.m:93-96), which differs in the foreground test of phase 1
// alone; of3d_mask_largest: the largest component alone (plot_figure2_movie.ipynb cell 1:
// measure.label, the regions sorted by area, all but the first zeroed), which differs in what
// follows the counting phase.  Connected components by label-equivalence union-find: every
// component ends rooted at its smallest linear index, so the component sizes, the counts and
// the kept mask are integers fixed by the input alone, whatever the dispatch order.
// Stream-ordered end to end: one launch per phase, nothing returns to the host, no workgroup
// waits for another (the union loop only retries its own atomicMin).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "summary_host.hpp"

namespace {

using u32 = unsigned;
using u64 = unsigned long long;

constexpr int kCclThreads = 256;  // a multiple of the wave: lane l of a wave holds voxel base + l
constexpr int kCclWalkBlocks = 4096;  // workgroups of the strided counting phases at most
constexpr u32 kBg = 0xFFFFFFFFu;  // background label
using of3dk::kMaxRoi;  // summary_host.hpp

// The 13 "backward" neighbours (negative linear offset) as rows (dz, dy) of three x offsets
// -1, 0, +1, and the in-row neighbour x-1.  Bit 3*row + (dx+1) of the neighbour mask selects
// (dz, dy, dx) of row `row`; bit 12 selects (0, 0, -1).
//   row 0: (-1,-1)  row 1: (-1, 0)  row 2: (-1,+1)  row 3: (0,-1)
constexpr int kRows = 4;
constexpr int kXBit = 12;
__host__ __device__ constexpr int row_dz(int r) { return r < 3 ? -1 : 0; }
__host__ __device__ constexpr int row_dy(int r) { return r < 3 ? r - 1 : -1; }

struct CclParams {
    int ny, nx;          // volume rows / columns (global index)
    int z0, y0, x0;      // the box's origin
    u32 dz, dy, dx;      // the box's extent
    u64 n;               // dz*dy*dx < 2^32 - 1
    u32 nbmask;          // neighbour mask (above)
    u32 roi;             // bit of keep
    u64 min_size;
};

struct Vox {
    u32 z, y, x;
    size_t g;  // index in the whole volume
};

__device__ __forceinline__ Vox locate(const CclParams& P, u32 i) {
    Vox v;
    const u32 row = i / P.dx;
    v.x = i - row * P.dx;
    v.z = row / P.dy;
    v.y = row - v.z * P.dy;
    v.g = ((size_t)(P.z0 + v.z) * P.ny + (P.y0 + v.y)) * P.nx + (P.x0 + v.x);
    return v;
}

// the x-runs of foreground lanes of this wave: bit l of `start` is set where lane l begins a
// run (first lane, first column of a row, or a background lane to its left)
__device__ __forceinline__ u64 run_starts(u64 fg, u64 row_start) { return fg & (~(fg << 1) | row_start | 1ull); }

__device__ __forceinline__ u32 load_label(const u32* L, u32 a) {
    return __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ u32 find_root(const u32* L, u32 a) {
    u32 p;
    while ((p = load_label(L, a)) != a) a = p;  // labels only decrease: terminates
    return a;
}

// The smaller root becomes the parent of the larger.  Lock-free: a lost atomicMin hands back
// the label that won, and the loop goes on from there; no thread waits for another's progress.
__device__ __forceinline__ void unite(u32* L, u32 a, u32 b) {
    for (;;) {
        a = find_root(L, a);
        b = find_root(L, b);
        if (a == b) return;
        if (a > b) {
            const u32 t = a;
            a = b;
            b = t;
        }
        const u32 old = atomicMin(&L[b], a);  // a < b
        if (old == b) return;
        b = old;
    }
}

// The foreground tests of phase 1, at the voxel's index in the whole volume.  FgSingle:
// of3d_mask_open's rel > thresh.  FgPair: of3d_mask_open_pair's joint test of two channels
// (plot_figure3_ROIfigures.m:93-95): the two threshold tests combined by OR or AND, and both
// fields above `floor`; a NaN field value fails the floor clause whatever the floor.
template <typename RelT>
struct FgSingle {
    const RelT* __restrict__ rel;
    const RelT* __restrict__ thr;
    __device__ __forceinline__ bool operator()(size_t g) const { return rel[g] > *thr; }  // NaN on either side: false
};

template <typename RelT>
struct FgPair {
    const RelT* __restrict__ rel0;
    const RelT* __restrict__ thr0;
    const RelT* __restrict__ rel1;
    const RelT* __restrict__ thr1;
    double floor;
    int combine;  // 0: OR, 1: AND
    __device__ __forceinline__ bool operator()(size_t g) const {
        const RelT a = rel0[g], b = rel1[g];
        const bool p0 = a > *thr0, p1 = b > *thr1;
        return (combine ? (p0 && p1) : (p0 || p1)) && (double)a > floor && (double)b > floor;
    }
};

// Phase 1: label[i] = first index of i's x-run inside its wave (foreground), kBg (background);
// size[i] = 0.
template <typename Fg>
__global__ __launch_bounds__(kCclThreads) void k_ccl_init(Fg is_fg, CclParams P, u32* __restrict__ label,
                                                          u32* __restrict__ size) {
    const u64 i64 = (u64)blockIdx.x * kCclThreads + threadIdx.x;
    const bool in = i64 < P.n;
    const u32 i = (u32)i64;
    bool fg = false, first = false;
    if (in) {
        const Vox v = locate(P, i);
        fg = is_fg(v.g);
        first = v.x == 0;
    }
    const u64 b = __ballot(fg), rs = __ballot(first);
    if (!in) return;
    const int lane = threadIdx.x & 63;
    u32 l = kBg;
    if (fg) {
        const u64 upto = run_starts(b, rs) & (~0ull >> (63 - lane));  // run starts at or below this lane
        l = i - (u32)(lane - (63 - __clzll((long long)upto)));
    }
    label[i] = l;
    size[i] = 0;
}

// Phase 2: every foreground voxel unites itself with its foreground backward neighbours.  In
// a row (dz, dy) above, a foreground centre is joined to its own x neighbours by their run, so
// the centre alone is enough where it is foreground (every connectivity that allows a diagonal
// of the row also allows its centre); the in-row neighbour x-1 is already this voxel's run
// unless the voxel is the first lane of its wave.
__global__ __launch_bounds__(kCclThreads) void k_ccl_merge(CclParams P, u32* __restrict__ label) {
    const u64 i64 = (u64)blockIdx.x * kCclThreads + threadIdx.x;
    if (i64 >= P.n) return;
    const u32 i = (u32)i64;
    if (load_label(label, i) == kBg) return;
    const Vox v = locate(P, i);
    if ((P.nbmask >> kXBit & 1) && (threadIdx.x & 63) == 0 && v.x > 0 && load_label(label, i - 1) != kBg)
        unite(label, i, i - 1);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const u32 m = P.nbmask >> (3 * r) & 7u;
        if (!m) continue;
        const int dz = row_dz(r), dy = row_dy(r);
        if ((dz < 0 && v.z == 0) || (dy < 0 && v.y == 0) || (dy > 0 && v.y + 1 >= P.dy)) continue;
        // the row's centre: i + (dz*dy_extent + dy) * dx_extent, below i
        const u32 c = i - (u32)(-(dz * (int64_t)P.dy + dy) * (int64_t)P.dx);
        if ((m & 2u) && load_label(label, c) != kBg) {
            unite(label, i, c);
            continue;
        }
        if ((m & 1u) && v.x > 0 && load_label(label, c - 1) != kBg) unite(label, i, c - 1);
        if ((m & 4u) && v.x + 1 < P.dx && load_label(label, c + 1) != kBg) unite(label, i, c + 1);
    }
}

// Phase 3 + 4: label[i] = root(i) (the component's smallest index) and size[root] = the
// component's voxels; n_mask and n_components.  A fixed number of workgroups walks the box; a
// wave counts its lanes per distinct root with ballots and carries one (root, count) pair from
// step to step, adding it to size[] only when the root changes: a component that fills the
// box costs a few atomics per wave instead of one per run (same-address atomics serialise).
__global__ __launch_bounds__(kCclThreads) void k_ccl_count(CclParams P, u32* __restrict__ label,
                                                           u32* __restrict__ size, u64* __restrict__ counts) {
    __shared__ u32 s_mask, s_comp;
    if (threadIdx.x == 0) s_mask = s_comp = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    u32 n_mask = 0, n_comp = 0;          // the wave's totals
    u32 pend_root = kBg, pend_len = 0;   // the wave's pending addition to size[]
    const u64 stride = (u64)gridDim.x * kCclThreads;
    for (u64 base = (u64)blockIdx.x * kCclThreads; base < P.n; base += stride) {
        const u64 i64 = base + threadIdx.x;
        const u32 i = (u32)i64;
        u32 root = kBg;
        if (i64 < P.n && load_label(label, i) != kBg) {
            root = find_root(label, i);
            label[i] = root;  // a concurrent reader sees the old parent or the root: both lead to the root
        }
        const bool fg = root != kBg;
        u64 todo = __ballot(fg);
        n_mask += (u32)__popcll(todo);
        n_comp += (u32)__popcll(__ballot(fg && root == i));
        while (todo) {  // one turn per distinct root among the wave's lanes
            const u32 r = (u32)__shfl((int)root, __builtin_ctzll(todo), 64);
            const u64 same = __ballot(fg && root == r);
            todo &= ~same;
            const u32 c = (u32)__popcll(same);
            if (r == pend_root) {
                pend_len += c;
            } else {
                if (pend_len && lane == 0) atomicAdd(&size[pend_root], pend_len);
                pend_root = r, pend_len = c;
            }
        }
    }
    if (lane == 0) {
        if (pend_len) atomicAdd(&size[pend_root], pend_len);
        if (n_mask) atomicAdd(&s_mask, n_mask);
        if (n_comp) atomicAdd(&s_comp, n_comp);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_mask) atomicAdd(&counts[0], (u64)s_mask);
        if (s_comp) atomicAdd(&counts[1], (u64)s_comp);
    }
}

// Phase 5: bit roi of keep where the component has min_size voxels; n_components_kept, n_kept.
// Another box's launch writes another bit of the same element, so the owning thread's plain
// read-modify-write is enough.
__global__ __launch_bounds__(kCclThreads) void k_ccl_write(CclParams P, const u32* __restrict__ label,
                                                           const u32* __restrict__ size, uint16_t* __restrict__ keep,
                                                           u64* __restrict__ counts) {
    __shared__ u32 s_kept, s_comp;
    if (threadIdx.x == 0) s_kept = s_comp = 0;
    __syncthreads();
    u32 n_kept = 0, n_comp = 0;  // the wave's totals
    const u64 stride = (u64)gridDim.x * kCclThreads;
    for (u64 base = (u64)blockIdx.x * kCclThreads; base < P.n; base += stride) {
        const u64 i64 = base + threadIdx.x;
        const u32 i = (u32)i64;
        bool kept = false, root_kept = false;
        if (i64 < P.n) {
            const u32 root = label[i];
            if (root != kBg && (u64)size[root] >= P.min_size) {
                kept = true;
                root_kept = root == i;
                const size_t g = locate(P, i).g;
                keep[g] = (uint16_t)(keep[g] | (1u << P.roi));
            }
        }
        n_kept += (u32)__popcll(__ballot(kept));
        n_comp += (u32)__popcll(__ballot(root_kept));
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_kept) atomicAdd(&s_kept, n_kept);
        if (n_comp) atomicAdd(&s_comp, n_comp);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_comp) atomicAdd(&counts[2], (u64)s_comp);
        if (s_kept) atomicAdd(&counts[3], (u64)s_kept);
    }
}

// Phase 5 of of3d_mask_largest: every root offers (size << 32) | (kBg - root) to the box's word
// `best` (zeroed on the stream).  The maximum is the largest component, among equals the one of
// the smallest root: a function of the input alone, whatever the order of the offers.  A
// thread keeps the largest of its own offers, a wave the largest of its lanes': one atomicMax
// per wave that saw a root.
__global__ __launch_bounds__(kCclThreads) void k_ccl_select(CclParams P, const u32* __restrict__ label,
                                                            const u32* __restrict__ size, u64* __restrict__ best) {
    u64 key = 0;  // a root's size is at least 1: 0 stands for "no root"
    const u64 stride = (u64)gridDim.x * kCclThreads;
    for (u64 i64 = (u64)blockIdx.x * kCclThreads + threadIdx.x; i64 < P.n; i64 += stride) {
        const u32 i = (u32)i64;
        if (label[i] != i) continue;
        const u64 k = ((u64)size[i] << 32) | (u64)(kBg - i);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_down(key, off, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

// Phase 6 of of3d_mask_largest: bit roi of keep where the voxel's root is the winner of
// `best`; n_components_kept (0 or 1) and n_kept (the winner's size) by one thread.
__global__ __launch_bounds__(kCclThreads) void k_ccl_write_largest(CclParams P, const u32* __restrict__ label,
                                                                   const u64* __restrict__ best,
                                                                   uint16_t* __restrict__ keep,
                                                                   u64* __restrict__ counts) {
    const u64 b = *best;
    if (!b) return;  // an empty mask keeps nothing; the counts stay 0
    const u32 winner = kBg - (u32)b;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[2] = 1, counts[3] = b >> 32;
    const u64 stride = (u64)gridDim.x * kCclThreads;
    for (u64 i64 = (u64)blockIdx.x * kCclThreads + threadIdx.x; i64 < P.n; i64 += stride) {
        const u32 i = (u32)i64;
        if (label[i] != winner) continue;
        const size_t g = locate(P, i).g;
        keep[g] = (uint16_t)(keep[g] | (1u << P.roi));
    }
}

// bits of the neighbour mask for a connectivity: a neighbour belongs to it when its number of
// non-zero offsets is at most 1 (4, 6), 2 (8, 18) or 3 (26)
u32 neighbour_mask(int connectivity) {
    const int max_nz = (connectivity == 4 || connectivity == 6) ? 1 : (connectivity == 26 ? 3 : 2);
    u32 m = 1u << kXBit;  // (0, 0, -1): one non-zero offset
    for (int r = 0; r < kRows; ++r)
        for (int dx = -1; dx <= 1; ++dx)
            if ((row_dz(r) != 0) + (row_dy(r) != 0) + (dx != 0) <= max_nz) m |= 1u << (3 * r + dx + 1);
    return m;
}

// the boxes as of3d_flow_summary validates them; vox[r] = voxels of box r
int check_boxes(const int64_t* rois, int n_roi, const int64_t dims[3], int64_t* vox) {
    if (of3dk::check_roi_count(rois, n_roi) != 0) return -1;
    for (int r = 0; r < n_roi; ++r) {
        vox[r] = 1;
        for (int a = 0; a < 3; ++a) {
            const int64_t ext = of3dk::box_extent(rois, r, a, dims);
            if (ext < 0) return -1;
            vox[r] *= ext;  // three factors below 2^31 each: the first two fit, the third is checked
            if (a == 1 && vox[r] >= (int64_t)kBg) break;
        }
        if (vox[r] >= (int64_t)kBg)
            return of3dk::set_error(("of3d: ROI " + std::to_string(r) + " has 2^32 - 1 voxels or more").c_str());
    }
    return 0;
}

// Everything of an opening but the argument checks of its foreground test: the phases per box,
// phase 1 with `is_fg` (of3d_mask_open and of3d_mask_open_pair differ in nothing else).
// largest (of3d_mask_largest): the selection and its write phase in place of phase 5.
template <typename Fg>
int open_launch(Fg is_fg, int64_t nz, int64_t ny, int64_t nx, const int64_t* rois, int n_roi, int64_t min_size,
                int connectivity, uint16_t* d_keep, int64_t* d_counts, void* workspace, void* stream,
                bool largest = false) {
    if (nz < 1 || ny < 1 || nx < 1 || nz > INT32_MAX || ny > INT32_MAX || nx > INT32_MAX)
        return of3dk::set_error("of3d: mask dims must lie in [1, 2^31)");
    if (min_size < 1) return of3dk::set_error("of3d: min_size must be at least 1");
    if (nz == 1 ? (connectivity != 4 && connectivity != 8)
                : (connectivity != 6 && connectivity != 18 && connectivity != 26))
        return of3dk::set_error("of3d: connectivity must be 4 or 8 for a 2D volume (nz == 1), 6, 18 or 26 for a 3D one");
    const int64_t dims[3] = {nz, ny, nx};
    int64_t vox[kMaxRoi], most = 0;
    if (check_boxes(rois, n_roi, dims, vox) != 0) return -1;
    for (int r = 0; r < n_roi; ++r) most = vox[r] > most ? vox[r] : most;
    hipStream_t s = (hipStream_t)stream;
    u32* label = (u32*)workspace;
    u32* size = label + most;
    u64* best = (u64*)(size + most);  // of3d_mask_largest: one word per box behind the sizes
    if (largest) OF3DK_HIP(hipMemsetAsync(best, 0, (size_t)n_roi * sizeof(u64), s));
    OF3DK_HIP(hipMemsetAsync(d_keep, 0, (size_t)nz * ny * nx * sizeof(uint16_t), s));
    OF3DK_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_roi * 4 * sizeof(int64_t), s));
    for (int r = 0; r < n_roi; ++r) {
        CclParams P;
        memset(&P, 0, sizeof(P));
        P.ny = (int)ny, P.nx = (int)nx;
        P.z0 = (int)rois[r * 6], P.y0 = (int)rois[r * 6 + 2], P.x0 = (int)rois[r * 6 + 4];
        P.dz = (u32)(rois[r * 6 + 1] - rois[r * 6]), P.dy = (u32)(rois[r * 6 + 3] - rois[r * 6 + 2]);
        P.dx = (u32)(rois[r * 6 + 5] - rois[r * 6 + 4]);
        P.n = (u64)vox[r];
        P.nbmask = neighbour_mask(connectivity);
        P.roi = (u32)r;
        P.min_size = (u64)min_size;
        const dim3 grid((unsigned)((P.n + kCclThreads - 1) / kCclThreads)), block(kCclThreads);
        u64* counts = (u64*)d_counts + (size_t)r * 4;
        hipLaunchKernelGGL(k_ccl_init<Fg>, grid, block, 0, s, is_fg, P, label, size);
        hipLaunchKernelGGL(k_ccl_merge, grid, block, 0, s, P, label);
        // the counting phases: a bounded grid that strides over the box (one atomic per workgroup
        // and count into the result, not one per 256 voxels)
        const dim3 walk(grid.x < (unsigned)kCclWalkBlocks ? grid.x : (unsigned)kCclWalkBlocks);
        hipLaunchKernelGGL(k_ccl_count, walk, block, 0, s, P, label, size, counts);
        if (largest) {
            hipLaunchKernelGGL(k_ccl_select, walk, block, 0, s, P, (const u32*)label, (const u32*)size, best + r);
            hipLaunchKernelGGL(k_ccl_write_largest, walk, block, 0, s, P, (const u32*)label, (const u64*)(best + r),
                               d_keep, counts);
        } else {
            hipLaunchKernelGGL(k_ccl_write, walk, block, 0, s, P, (const u32*)label, (const u32*)size, d_keep, counts);
        }
    }
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

size_t of3d_mask_open_workspace_bytes(const int64_t* rois, int n_roi) {
    int64_t vox[kMaxRoi], most = 0;
    if (check_boxes(rois, n_roi, nullptr, vox) != 0) return 0;
    for (int r = 0; r < n_roi; ++r) most = vox[r] > most ? vox[r] : most;
    return (size_t)most * 2 * sizeof(u32);
}

int of3d_mask_open(const void* d_rel, int rel_f64, int64_t nz, int64_t ny, int64_t nx, const void* d_thresh,
                   const int64_t* rois, int n_roi, int64_t min_size, int connectivity, uint16_t* d_keep,
                   int64_t* d_counts, void* workspace, void* stream) {
    if (!d_rel || !d_thresh || !rois || !d_keep || !d_counts || !workspace)
        return of3dk::set_error("of3d: null argument");
    if (rel_f64)
        return open_launch(FgSingle<double>{(const double*)d_rel, (const double*)d_thresh}, nz, ny, nx, rois, n_roi,
                           min_size, connectivity, d_keep, d_counts, workspace, stream);
    return open_launch(FgSingle<float>{(const float*)d_rel, (const float*)d_thresh}, nz, ny, nx, rois, n_roi,
                       min_size, connectivity, d_keep, d_counts, workspace, stream);
}

size_t of3d_mask_largest_workspace_bytes(const int64_t* rois, int n_roi) {
    const size_t open_bytes = of3d_mask_open_workspace_bytes(rois, n_roi);
    return open_bytes ? open_bytes + (size_t)n_roi * sizeof(u64) : 0;
}

int of3d_mask_largest(const void* d_rel, int rel_f64, int64_t nz, int64_t ny, int64_t nx, const void* d_thresh,
                      const int64_t* rois, int n_roi, int connectivity, uint16_t* d_keep, int64_t* d_counts,
                      void* workspace, void* stream) {
    if (!d_rel || !d_thresh || !rois || !d_keep || !d_counts || !workspace)
        return of3dk::set_error("of3d: null argument");
    if (rel_f64)
        return open_launch(FgSingle<double>{(const double*)d_rel, (const double*)d_thresh}, nz, ny, nx, rois, n_roi,
                           1, connectivity, d_keep, d_counts, workspace, stream, true);
    return open_launch(FgSingle<float>{(const float*)d_rel, (const float*)d_thresh}, nz, ny, nx, rois, n_roi, 1,
                       connectivity, d_keep, d_counts, workspace, stream, true);
}

int of3d_mask_open_pair(const void* d_rel0, const void* d_thresh0, const void* d_rel1, const void* d_thresh1,
                        int rel_f64, double floor, int combine, int64_t nz, int64_t ny, int64_t nx,
                        const int64_t* rois, int n_roi, int64_t min_size, int connectivity, uint16_t* d_keep,
                        int64_t* d_counts, void* workspace, void* stream) {
    if (!d_rel0 || !d_thresh0 || !d_rel1 || !d_thresh1 || !rois || !d_keep || !d_counts || !workspace)
        return of3dk::set_error("of3d: null argument");
    if (combine != 0 && combine != 1) return of3dk::set_error("of3d: combine must be 0 (OR) or 1 (AND)");
    if (floor != floor) return of3dk::set_error("of3d: floor must not be NaN (-INFINITY switches the clause off)");
    if (rel_f64)
        return open_launch(FgPair<double>{(const double*)d_rel0, (const double*)d_thresh0, (const double*)d_rel1,
                                          (const double*)d_thresh1, floor, combine},
                           nz, ny, nx, rois, n_roi, min_size, connectivity, d_keep, d_counts, workspace, stream);
    return open_launch(FgPair<float>{(const float*)d_rel0, (const float*)d_thresh0, (const float*)d_rel1,
                                     (const float*)d_thresh1, floor, combine},
                       nz, ny, nx, rois, n_roi, min_size, connectivity, d_keep, d_counts, workspace, stream);
}

}  // extern "C"

#pragma once
// summary_dev.hpp — the per-voxel device helpers shared by the frame summary (kt_summary.hip:
// k_sum_boxes), the projected flow (kt_axes.hip: k_proj_boxes) and the magnitude-weighted
// histograms (kt_whist.hip: k_whist_boxes): one statement of the masking arithmetic, the
// histogram bin search and the walk over a box, so the passes cannot drift apart.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace of3dk {

// The workgroup partition of a box's reduction (k_sum_boxes, k_proj_boxes, k_whist_boxes): workgroup b of nb
// walks rows [b*R/nb, (b+1)*R/nb) of the box's R = dz*dy rows.  nb is a function of the box
// alone (never of the device), so the summation order is fixed.
constexpr int kSumThreads = 512, kSumWaves = kSumThreads / 64;
constexpr int kSumMaxBlocks = 1024;        // workgroups (workspace slots) per box at most
constexpr int64_t kSumVoxPerBlock = 8192;  // a workgroup's share of a box at least
inline int64_t sum_workgroups(int64_t vox, int64_t rows) {
    int64_t nb = (vox + kSumVoxPerBlock - 1) / kSumVoxPerBlock;
    nb = nb > kSumMaxBlocks ? kSumMaxBlocks : nb;
    return nb > rows ? rows : nb;
}

// np.histogram(v, bins=e): e[i] <= v < e[i+1], the last bin closed; -1: dropped (outside, NaN)
__device__ __forceinline__ int find_bin(const double* e, int nb, double v) {
    if (!(v >= e[0] && v <= e[nb])) return -1;
    int lo = 0, hi = nb;  // e[lo] <= v, and v < e[hi] or hi == nb
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v >= e[mid])
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// example_analysis_script.ipynb cell 5 for one component: v * mask (numpy: v * bool mask),
// exact zeros -> NaN, then (v * scale) / tscale
__device__ __forceinline__ double masked_velocity(double v, double m, double scale, double tscale) {
    v = v * m;
    if (v == 0.0) v = __builtin_nan("");
    return (v * scale) / tscale;
}

// Quantity q of a valid voxel in of3d_flow_summary's order (0 vx, 1 vy, 2 vz, 3 magnitude,
// 4 theta, 5 phi), from the physical velocities, the magnitude and h = sqrt(vx^2 + vy^2): the
// values k_sum_boxes bins (kt_whist.hip bins the same ones, one quantity per workgroup)
__device__ __forceinline__ double quantity_value(int q, double vxp, double vyp, double vzp, double mag, double h) {
    switch (q) {
        case 0: return vxp;
        case 1: return vyp;
        case 2: return vzp;
        case 3: return mag;
        case 4: return atan2(vyp, vxp);
        default: return atan(vzp / h);
    }
}

// A thread's voxel as (z, y, x) inside a box of dy rows of dx voxels per plane, advanced by
// `threads` voxels per step without divisions: x by threads % dx with a carry into the row,
// the row by threads / dx.
struct BoxWalk {
    unsigned x, y, z;
    unsigned dx, dy, step_x, step_y, step_z;

    // the voxel `tid` voxels after the first of row `row0` (rows counted over the whole box)
    __device__ __forceinline__ BoxWalk(unsigned dy_, unsigned dx_, long long row0, unsigned tid, unsigned threads)
        : dx(dx_), dy(dy_) {
        const unsigned step_r = threads / dx;
        step_x = threads % dx;
        step_y = step_r % dy, step_z = step_r / dy;
        x = tid % dx;
        const long long row = row0 + tid / dx;
        y = (unsigned)(row % dy), z = (unsigned)(row / dy);
    }

    __device__ __forceinline__ void advance() {
        x += step_x;
        unsigned c = x >= dx;
        x -= c ? dx : 0;
        y += step_y + c;
        c = y >= dy;
        y -= c ? dy : 0;
        z += step_z + c;
    }
};

}  // namespace of3dk

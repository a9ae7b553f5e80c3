#pragma once
// summary_dev.hpp — the per-voxel device helpers shared by the frame summary (kt_summary.hip:
// k_sum_boxes), the projected flow (kt_axes.hip: k_proj_boxes), the magnitude-weighted
// histograms (kt_whist.hip: k_whist_boxes) and the two-channel comparison (kt_pair.hip:
// k_pair_boxes): one statement of the masking arithmetic, the histogram bin search, the walk
// over a box and the plan of the boxes' workgroups, so the passes cannot drift apart.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"

namespace of3dk {

// The workgroup partition of a box's reduction (k_sum_boxes, k_proj_boxes, k_whist_boxes, k_pair_boxes): workgroup b of nb
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

// The boxes of a pass with per-workgroup workspace slots (of3d_flow_whist, of3d_flow_pair) as
// of3d_flow_summary validates them (dims NULL: against 2^31 alone) and their workgroups;
// soff_out[r]: the first slot word of box r, slot_words: the sum over the boxes of
// workgroups * wg_words.
inline int plan_boxes(const int64_t* rois, int n_roi, const int64_t* dims, int wg_words, int* nb_out,
                      long long* soff_out, size_t* slot_words) {
    constexpr int kMaxRoi = OF3D_SUMMARY_MAX_ROI;
    if (!rois) return set_error("of3d: null argument");
    if (n_roi < 1 || n_roi > kMaxRoi) return set_error("of3d: 1 to 16 ROI boxes");
    size_t words = 0;
    for (int r = 0; r < n_roi; ++r) {
        int64_t ext[3];
        for (int a = 0; a < 3; ++a) {
            const int64_t b0 = rois[r * 6 + 2 * a], b1 = rois[r * 6 + 2 * a + 1];
            if (b0 < 0 || b0 >= b1 || b1 > (dims ? dims[a] : (int64_t)INT32_MAX))
                return set_error(("of3d: ROI " + std::to_string(r) + " is empty or outside the volume").c_str());
            ext[a] = b1 - b0;
        }
        // a function of the box alone (never of the device): the summation order is fixed
        const int64_t rows = ext[0] * ext[1];  // < 2^62
        const int64_t big = INT64_MAX / 2;     // stands for any larger voxel count: the cap decides
        const int64_t nb = sum_workgroups(ext[2] > big / rows ? big : rows * ext[2], rows);
        // a workgroup's share, at most ceil(rows / nb) rows of ext[2] voxels, must stay below lim
        const int64_t lim = ((int64_t)1 << 31) - 4 * kSumThreads;
        if ((rows + nb - 1) / nb >= (lim + ext[2] - 1) / ext[2])
            return set_error("of3d: ROI too large (2^31 voxels per workgroup)");
        if (nb_out) nb_out[r] = (int)nb;
        if (soff_out) soff_out[r] = (long long)words;
        words += (size_t)nb * wg_words;
    }
    *slot_words = words;
    return 0;
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

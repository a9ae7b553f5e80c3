// kt_spread.hip — the spread of the flow about a centre (of3d_flow_spread): per box the sums of
// squares and cross products of the deviations of vx, vy, vz and the magnitude from a centre,
// the sums of sin / cos of phi, and the extremes — what the reference's validation figure
// (plot_FigureS1_translation.ipynb, cell "Calculations over time": np.nanstd of vx, vy, vz and
// the speed, the circular std of theta and phi) reduces a frame to.  A pass of its own after
// of3d_flow_summary, as k_whist_boxes (kt_whist.hip) is: the deviations are centred, and the
// centre of a box (its mean) exists only once the summary's final kernel has run; it is read
// here from the summary's device result, nothing returns to the host.  The per-voxel
// arithmetic, the walk, the workgroup partition and the reduction are summary_dev.hpp's.
//   k_spread_boxes  per-thread accumulators, reduce_to_slot<9>, the extremes beside them
//   k_spread_final  a box's slots in index order; the centre used
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "summary_dev.hpp"

namespace {

using u64 = unsigned long long;

using of3dk::kSumThreads, of3dk::kSumWaves, of3dk::kSumMaxBlocks, of3dk::kMaxRoi, of3dk::plan_boxes;  // summary_host.hpp
constexpr int kNQ = OF3D_SUMMARY_QUANTITIES;
constexpr int kRoiWords = OF3D_SPREAD_ROI_WORDS;
constexpr int kNSum = 9;  // dvx^2 dvy^2 dvz^2 dmag^2 dvx*dvy dvx*dvz dvy*dvz sin(phi) cos(phi)
constexpr int kNExt = 8;  // min vx vy vz mag, max vx vy vz mag
constexpr int kSlot = kNSum + kNExt;  // a workgroup's workspace slot: the sums, then the extremes
static_assert(kRoiWords == 1 + 4 + kNSum + kNExt);

// Workspace: the slots [roi][workgroup][17].
struct SpParams : of3dk::BoxParams {
    long long soff[kMaxRoi];  // first slot word of the box: sum over earlier boxes of nb * 17
    int given;                // the centre is c (the same for every box), not the box's mean
    int sum_words;            // words per box of the summary's result
    double c[4];              // vx vy vz magnitude
    double sxy, sz, st;
};

// Component q (0 vx, 1 vy, 2 vz, 3 magnitude) of box roi's centre: the given one, or the box's
// mean sum_q / n_valid from of3d_flow_summary's result (its sums: magnitude, vx, vy, vz) — one
// IEEE division; n_valid == 0 gives 0 / 0 = NaN.
__device__ __forceinline__ double box_center(const SpParams& P, const u64* __restrict__ summary, int roi, int q) {
    if (P.given) return P.c[q];
    const u64* sr = summary + of3dk::kSummaryHead + (size_t)roi * P.sum_words;
    return __longlong_as_double((long long)sr[2 + (q + 1) % 4]) / (double)(long long)sr[0];
}

// Lane 0 returns the minimum (Max: the maximum) of the wave's 64 lanes, all of them active.
// No NaN comes here (a valid voxel has none), so the order of the comparisons does not matter.
template <bool Max>
__device__ __forceinline__ double wave_extreme(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = (Max ? o > v : o < v) ? o : v;
    }
    return v;
}

// Grid (max workgroups of a box, n_roi).  Masked: the mask factor of a voxel is bit `roi` of keep
// (of3d_mask_open) instead of rel > thr.
template <typename VT, typename RelT, bool Masked>
__global__ __launch_bounds__(kSumThreads) void k_spread_boxes(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                              const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                              const RelT* __restrict__ thr_p,
                                                              const uint16_t* __restrict__ keep, SpParams P,
                                                              const u64* __restrict__ summary,
                                                              double* __restrict__ slots, u64* __restrict__ result) {
    const int roi = blockIdx.y, nb = P.nb[roi];
    if ((int)blockIdx.x >= nb) return;
    __shared__ unsigned nvalid_s;
    __shared__ double wsum[kSumWaves][kNSum];
    __shared__ double wext[kSumWaves][kNExt];
    if (threadIdx.x == 0) nvalid_s = 0;
    __syncthreads();

    of3dk::BoxShare sh = of3dk::box_share(P, roi, nb);
    const of3dk::FlowFields<VT, RelT, Masked> F{vx,    vy,   vz,   rel, keep,         Masked ? 0.0 : (double)*thr_p,
                                                P.sxy, P.sz, P.st, roi, vz != nullptr};
    const bool is3 = F.is3;
    const double cx = box_center(P, summary, roi, 0), cy = box_center(P, summary, roi, 1);
    const double cz = box_center(P, summary, roi, 2), cm = box_center(P, summary, roi, 3);
    const double inf = __builtin_inf();
    double acc[kNSum] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double ext[kNExt] = {inf, inf, inf, inf, -inf, -inf, -inf, -inf};
    unsigned nvalid = 0;

    of3dk::for_valid_voxels(F, sh, [&](const of3dk::Voxel& v, unsigned, unsigned, unsigned) {
        const double vxp = v.vxp, vyp = v.vyp, vzp = v.vzp, mag = sqrt(v.sq);
        const double dx = vxp - cx, dy = vyp - cy, dz = is3 ? vzp - cz : 0.0, dm = mag - cm;
        ++nvalid;
        acc[0] += dx * dx;
        acc[1] += dy * dy;
        acc[2] += dz * dz;
        acc[3] += dm * dm;
        acc[4] += dx * dy;
        acc[5] += dx * dz;
        acc[6] += dy * dz;
        if (is3) {  // phi = atan(vz / h): sin = vz / mag, cos = h / mag, as the summary's sin(theta) = vy / h
            acc[7] += vzp / mag;
            acc[8] += sqrt(v.xy2) / mag;
        }
        ext[0] = vxp < ext[0] ? vxp : ext[0];
        ext[1] = vyp < ext[1] ? vyp : ext[1];
        ext[2] = vzp < ext[2] ? vzp : ext[2];
        ext[3] = mag < ext[3] ? mag : ext[3];
        ext[4] = vxp > ext[4] ? vxp : ext[4];
        ext[5] = vyp > ext[5] ? vyp : ext[5];
        ext[6] = vzp > ext[6] ? vzp : ext[6];
        ext[7] = mag > ext[7] ? mag : ext[7];
    });

    if (nvalid) atomicAdd(&nvalid_s, nvalid);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kNExt; ++k) {
        const double v = k < 4 ? wave_extreme<false>(ext[k]) : wave_extreme<true>(ext[k]);
        if (lane == 0) wext[wave][k] = v;
    }
    double* slot = slots + P.soff[roi] + (long long)blockIdx.x * kSlot;
    of3dk::reduce_to_slot(acc, wsum, slot);  // its barrier also publishes wext and nvalid_s
    const int k = (int)threadIdx.x - 64;     // the second wave folds the extremes
    if (k >= 0 && k < kNExt) {
        double v = wext[0][k];
        for (int j = 1; j < kSumWaves; ++j) v = (k < 4 ? wext[j][k] < v : wext[j][k] > v) ? wext[j][k] : v;
        slot[kNSum + k] = v;
    }
    if (threadIdx.x == 0 && nvalid_s) atomicAdd(&result[(size_t)roi * kRoiWords], (u64)nvalid_s);
}

// Grid (n_roi, 2).  Workgroup (r, 0): box r's nine sums, its slots staged in LDS and added in
// index order, and the centre used.  Workgroup (r, 1): the extremes of its slots (NaN for a box
// without a valid voxel: n_valid is complete, k_spread_boxes ran before on the stream).
__global__ __launch_bounds__(of3dk::kFinalThreads) void k_spread_final(const double* __restrict__ slots, SpParams P,
                                                                       const u64* __restrict__ summary,
                                                                       u64* __restrict__ result) {
    __shared__ double s[kSumMaxBlocks * kNSum];
    const int roi = blockIdx.x, nb = P.nb[roi];
    u64* rr = result + (size_t)roi * kRoiWords;
    const double* src = slots + P.soff[roi];
    if (blockIdx.y == 0) {
        of3dk::add_slots<kNSum, kSlot>(src, nb, s, rr + 5);
        if (threadIdx.x >= 64 && threadIdx.x < 68)
            rr[1 + threadIdx.x - 64] = (u64)__double_as_longlong(box_center(P, summary, roi, threadIdx.x - 64));
        return;
    }
    for (int i = threadIdx.x; i < nb * kNExt; i += of3dk::kFinalThreads)
        s[i] = src[(size_t)(i / kNExt) * kSlot + kNSum + i % kNExt];
    __syncthreads();
    if (threadIdx.x < kNExt) {
        const int k = threadIdx.x;
        double v = s[k];
        for (int b = 1; b < nb; ++b) {
            const double o = s[b * kNExt + k];
            v = (k < 4 ? o < v : o > v) ? o : v;
        }
        if (rr[0] == 0) v = __builtin_nan("");
        rr[5 + kNSum + k] = (u64)__double_as_longlong(v);
    }
}

}  // namespace

extern "C" {

size_t of3d_flow_spread_result_bytes(int n_roi) {
    if (n_roi < 1 || n_roi > kMaxRoi) return 0;
    return (size_t)n_roi * kRoiWords * 8;
}

size_t of3d_flow_spread_workspace_bytes(const int64_t* rois, int n_roi) {
    size_t slot_words = 0;
    if (plan_boxes(rois, n_roi, nullptr, kSlot, nullptr, nullptr, &slot_words) != 0) return 0;
    return slot_words * sizeof(double);
}

int of3d_flow_spread(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                     int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                     double tscale, const int64_t* rois, int n_roi, const uint16_t* d_keep, const void* d_summary,
                     const int* summary_nbins, const double* center, void* d_result, void* workspace, void* stream) {
    if (!vx || !vy || !rois || !d_result || !workspace || (!d_keep && (!rel || !d_thresh)))
        return of3dk::set_error("of3d: null argument");
    if (of3dk::check_volume(nz, ny, nx, !vz) != 0) return -1;
    if (!center && !d_summary) return of3dk::set_error("of3d: a spread needs a center or the summary's result");
    if (!center && !of3dk::bins_ok<kNQ>(summary_nbins))
        return of3dk::set_error("of3d: the summary's nbins: 0 to 256 bins per quantity");
    SpParams P{};
    P.sxy = xyscale, P.sz = zscale, P.st = tscale;
    P.given = center != nullptr;
    if (center) {
        for (int q = 0; q < 4; ++q) P.c[q] = center[q];
        if (!vz) P.c[2] = 0.0;  // 2D: every vz term is 0
    } else {
        P.sum_words = of3dk::kSummaryRoiHead + of3dk::total_bins<kNQ>(summary_nbins);
    }
    const int64_t dims[3] = {nz, ny, nx};
    if (plan_boxes(rois, n_roi, dims, kSlot, P.nb, P.soff) != 0) return -1;
    const int max_nb = of3dk::fill_boxes(P, dims, rois, n_roi);
    hipStream_t s = (hipStream_t)stream;
    double* slots = (double*)workspace;
    u64* res = (u64*)d_result;
    const u64* sum = (const u64*)d_summary;
    OF3DK_HIP(hipMemsetAsync(d_result, 0, of3d_flow_spread_result_bytes(n_roi), s));
    const dim3 grid(max_nb, n_roi);
    of3dk::with_flow_types(v_f32, rel_f64, d_keep != nullptr, [&](auto vt, auto rt, auto masked_c) {
        using VT = decltype(vt);
        using RT = decltype(rt);
        constexpr bool M = decltype(masked_c)::value;
        hipLaunchKernelGGL((k_spread_boxes<VT, RT, M>), grid, dim3(kSumThreads), 0, s, (const VT*)vx, (const VT*)vy,
                           (const VT*)vz, (const RT*)rel, (const RT*)d_thresh, d_keep, P, sum, slots, res);
    });
    hipLaunchKernelGGL(k_spread_final, dim3(n_roi, 2), dim3(of3dk::kFinalThreads), 0, s, (const double*)slots, P, sum,
                       res);
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

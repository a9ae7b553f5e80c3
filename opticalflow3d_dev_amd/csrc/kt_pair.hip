// kt_pair.hip — two-channel comparison of one frame (of3d_flow_pair): the reference's figure 3
// (plot_figure3_ROIfigures.m:98-193, plot_figure3_ChannelCompare.m:142-164) reduces two
// channels' flows over the SAME voxels — those of the joint reliability mask
// (of3d_mask_open_pair, kt_ccl.hip) where both channels have a magnitude — to per-ROI circular
// means per channel and compares them.  Here one pass over both channels' fields gives, per
// box, each channel's eight of3d_flow_summary sums over the jointly valid voxels, eight cross
// sums (dot product, cosine of the angle between the flows, the magnitude moments, sin / cos of
// the in-plane angle difference, the endpoint difference) and four histograms.  The per-voxel
// arithmetic, the bin search, the walk and the workgroup partition are summary_dev.hpp's, the
// reduction contract is k_sum_boxes' (kt_summary.hip).
//   k_pair_boxes  24 sums in registers, the fixed shuffle tree, the waves in wave order, one
//                 workspace slot per workgroup; counts by integer atomics
//   k_pair_final  grid (box, group of 8 sums): a group's slots staged in LDS (64 KiB at most),
//                 added in workgroup-index order
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "summary_dev.hpp"

namespace {

using u64 = unsigned long long;

using of3dk::kSumThreads, of3dk::kSumWaves, of3dk::kSumMaxBlocks, of3dk::kMaxBins, of3dk::kMaxRoi, of3dk::plan_boxes;
constexpr int kNQ = OF3D_PAIR_QUANTITIES;  // 0 dot, 1 cosine, 2 dtheta, 3 dmagnitude
constexpr int kRoiHead = OF3D_PAIR_ROI_WORDS;
constexpr int kNSum = 24, kGroup = 8;  // sums per box; sums per workgroup of the final pass
constexpr size_t kEdgeWordsMax = (size_t)kNQ * (kMaxBins + 1);
static_assert(kRoiHead == 2 + kNSum && kNSum % kGroup == 0);

// Workspace: the edges (eo words), then the slots [roi][workgroup][24].
struct PairParams : of3dk::BoxParams {
    long long soff[kMaxRoi];  // first slot word of the box: sum over earlier boxes of nb * 24
    int nbins[kNQ];
    int eoff[kNQ];  // first edge of the quantity in the workspace's edge array
    int hoff[kNQ];  // first bin of the quantity in a box's histogram words
    int ntot;       // bins of a box, all quantities
    double sxy, sz, st;
};

// Grid (max workgroups of a box, n_roi).  InPlane: no vz fields, magnitude = sqrt(vx^2 + vy^2)
// for any nz.  The voxel loop runs the same trips in every lane (tail lanes carry mask factor
// 0), so the ballot of the wave-uniform skip sees every lane.
template <typename VT, bool InPlane>
__global__ __launch_bounds__(kSumThreads) void k_pair_boxes(
    const VT* __restrict__ vx0, const VT* __restrict__ vy0, const VT* __restrict__ vz0, const VT* __restrict__ vx1,
    const VT* __restrict__ vy1, const VT* __restrict__ vz1, const uint16_t* __restrict__ keep, PairParams P,
    const double* __restrict__ edges_g, double* __restrict__ slots, u64* __restrict__ result) {
    const int roi = blockIdx.y, nb = P.nb[roi];
    if ((int)blockIdx.x >= nb) return;
    __shared__ double edges[kEdgeWordsMax];
    __shared__ unsigned hist[kNQ * kMaxBins];
    __shared__ unsigned nvalid_s;
    __shared__ double wsum[kSumWaves][kNSum];
    int ne = 0;
    for (int q = 0; q < kNQ; ++q) ne += P.nbins[q] ? P.nbins[q] + 1 : 0;
    for (int i = threadIdx.x; i < ne; i += kSumThreads) edges[i] = edges_g[i];
    for (int i = threadIdx.x; i < P.ntot; i += kSumThreads) hist[i] = 0;
    if (threadIdx.x == 0) nvalid_s = 0;
    __syncthreads();

    of3dk::BoxShare sh = of3dk::box_share(P, roi, nb);
    const long long count = sh.count;
    double acc[kNSum];
#pragma unroll
    for (int q = 0; q < kNSum; ++q) acc[q] = 0.0;
    unsigned nvalid = 0;

    constexpr int U = 4;
    for (long long e0 = 0; e0 < count; e0 += (long long)U * kSumThreads) {  // the same trips in every lane
        VT fx0[U], fy0[U], fz0[U], fx1[U], fy1[U], fz1[U];
        bool kept[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            fx0[u] = fy0[u] = fz0[u] = fx1[u] = fy1[u] = fz1[u] = (VT)0;  // past the end: mask factor 0, not valid
            kept[u] = false;
            if (e0 + threadIdx.x + (long long)u * kSumThreads < count) {
                const size_t i = sh.index();
                kept[u] = keep[i] >> roi & 1;
                fx0[u] = vx0[i];
                fy0[u] = vy0[i];
                fx1[u] = vx1[i];
                fy1[u] = vy1[i];
                if constexpr (!InPlane) {
                    fz0[u] = vz0[i];
                    fz1[u] = vz1[i];
                }
            }
            sh.w.advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double m = kept[u] ? 1.0 : 0.0;  // numpy: v * bool mask
            const double x0p = of3dk::masked_velocity((double)fx0[u], m, P.sxy, P.st);
            const double y0p = of3dk::masked_velocity((double)fy0[u], m, P.sxy, P.st);
            const double x1p = of3dk::masked_velocity((double)fx1[u], m, P.sxy, P.st);
            const double y1p = of3dk::masked_velocity((double)fy1[u], m, P.sxy, P.st);
            const double z0p = InPlane ? 0.0 : of3dk::masked_velocity((double)fz0[u], m, P.sz, P.st);
            const double z1p = InPlane ? 0.0 : of3dk::masked_velocity((double)fz1[u], m, P.sz, P.st);
            const double xy0 = x0p * x0p + y0p * y0p, xy1 = x1p * x1p + y1p * y1p;
            const double sq0 = InPlane ? xy0 : xy0 + z0p * z0p, sq1 = InPlane ? xy1 : xy1 + z1p * z1p;
            // badRows = isnan(mag0) | isnan(mag1): a sum of squares is NaN or >= 0, so its root
            // is NaN exactly where it is
            const bool valid = sq0 == sq0 && sq1 == sq1;
            if (!__ballot(valid)) continue;  // wave-uniform: no root, divide or atan2 where no lane is valid
            if (!valid) continue;
            const double mag0 = sqrt(sq0), mag1 = sqrt(sq1);
            const double h0 = sqrt(xy0), h1 = sqrt(xy1);
            const double sn0 = y0p / h0, cs0 = x0p / h0, sn1 = y1p / h1, cs1 = x1p / h1;
            ++nvalid;
            acc[0] += mag0;
            acc[1] += x0p;
            acc[2] += y0p;
            if constexpr (!InPlane) acc[3] += z0p;
            acc[4] += sn0;
            acc[5] += cs0;
            acc[6] += mag0 * sn0;
            acc[7] += mag0 * cs0;
            acc[8] += mag1;
            acc[9] += x1p;
            acc[10] += y1p;
            if constexpr (!InPlane) acc[11] += z1p;
            acc[12] += sn1;
            acc[13] += cs1;
            acc[14] += mag1 * sn1;
            acc[15] += mag1 * cs1;
            const double dxy = x0p * x1p + y0p * y1p;
            const double dot = InPlane ? dxy : dxy + z0p * z1p;
            const double mm = mag0 * mag1;
            const double cosine = dot / mm;  // not clamped: rounding may leave it a few ulp past +-1
            const double cosd = cs0 * cs1 + sn0 * sn1, sind = cs0 * sn1 - sn0 * cs1;
            const double ex = x1p - x0p, ey = y1p - y0p, ez = z1p - z0p;
            const double exy = ex * ex + ey * ey;
            const double diff = InPlane ? sqrt(exy) : sqrt(exy + ez * ez);
            acc[16] += dot;
            acc[17] += cosine;
            acc[18] += mm;
            acc[19] += mag0 * mag0;
            acc[20] += mag1 * mag1;
            acc[21] += sind;
            acc[22] += cosd;
            acc[23] += diff;
            auto put = [&](int q, double v) {
                const int b = of3dk::find_bin(edges + P.eoff[q], P.nbins[q], v);
                if (b >= 0) atomicAdd(&hist[P.hoff[q] + b], 1u);
            };
            if (P.nbins[0]) put(0, dot);
            if (P.nbins[1]) put(1, cosine);
            if (P.nbins[2]) put(2, atan2(sind, cosd));
            if (P.nbins[3]) put(3, mag1 - mag0);
        }
    }

    if (nvalid) atomicAdd(&nvalid_s, nvalid);
    of3dk::reduce_to_slot(acc, wsum, slots + P.soff[roi] + (long long)blockIdx.x * kNSum);
    u64* rr = result + (size_t)roi * (kRoiHead + P.ntot);
    if (threadIdx.x == 0 && nvalid_s) atomicAdd(&rr[0], (u64)nvalid_s);
    of3dk::flush_hist(hist, P.ntot, rr + kRoiHead);
}

// Grid (n_roi, 3): workgroup (r, g) stages sums 8g .. 8g+7 of box r's slots in LDS (at most
// 1024 x 8 doubles = 64 KiB) and adds each in workgroup-index order.
__global__ __launch_bounds__(of3dk::kFinalThreads) void k_pair_final(const double* __restrict__ slots, PairParams P,
                                                                     u64* __restrict__ result) {
    __shared__ double s[kSumMaxBlocks * kGroup];
    const int roi = blockIdx.x, g = blockIdx.y;
    u64* rr = result + (size_t)roi * (kRoiHead + P.ntot);
    of3dk::add_slots<kGroup, kNSum>(slots + P.soff[roi] + g * kGroup, P.nb[roi], s, rr + 2 + g * kGroup);
    if (g == 0 && threadIdx.x == 0) {
        const int* bx = P.box[roi];
        rr[1] = (u64)((long long)(bx[1] - bx[0]) * (bx[3] - bx[2]) * (bx[5] - bx[4]));
    }
}

}  // namespace

extern "C" {

size_t of3d_flow_pair_result_bytes(int n_roi, const int* nbins4) {
    if (n_roi < 1 || n_roi > kMaxRoi || !of3dk::bins_ok<kNQ>(nbins4)) return 0;
    return (size_t)n_roi * (kRoiHead + of3dk::total_bins<kNQ>(nbins4)) * 8;
}

size_t of3d_flow_pair_workspace_bytes(const int64_t* rois, int n_roi, const int* nbins4) {
    if (!of3dk::bins_ok<kNQ>(nbins4)) {
        of3dk::set_error("of3d: 0 to 256 bins per quantity");
        return 0;
    }
    size_t slot_words = 0;
    if (plan_boxes(rois, n_roi, nullptr, kNSum, nullptr, nullptr, &slot_words) != 0) return 0;
    return (of3dk::edge_words<kNQ>(nbins4) + slot_words) * sizeof(double);
}

int of3d_flow_pair(const void* vx0, const void* vy0, const void* vz0, const void* vx1, const void* vy1,
                   const void* vz1, int v_f32, int64_t nz, int64_t ny, int64_t nx, double xyscale, double zscale,
                   double tscale, const int64_t* rois, int n_roi, const uint16_t* d_keep, const int* nbins4,
                   const double* const* edges4, void* d_result, void* workspace, void* stream) {
    if (!vx0 || !vy0 || !vx1 || !vy1 || !rois || !d_keep || !d_result || !workspace)
        return of3dk::set_error("of3d: null argument");
    if (!vz0 != !vz1) return of3dk::set_error("of3d: vz of both channels or of neither (in-plane mode)");
    if (of3dk::check_volume(nz, ny, nx, false) != 0) return -1;
    if (!of3dk::bins_ok<kNQ>(nbins4)) return of3dk::set_error("of3d: 0 to 256 bins per quantity");
    PairParams P{};
    P.sxy = xyscale, P.sz = zscale, P.st = tscale;
    P.ntot = of3dk::total_bins<kNQ>(nbins4);
    const int64_t dims[3] = {nz, ny, nx};
    if (plan_boxes(rois, n_roi, dims, kNSum, P.nb, P.soff) != 0) return -1;
    const int max_nb = of3dk::fill_boxes(P, dims, rois, n_roi);
    double host_edges[kEdgeWordsMax];
    const int eo = of3dk::plan_hists<kNQ>(nbins4, edges4, P.nbins, P.eoff, P.hoff, host_edges);
    if (eo < 0) return -1;
    hipStream_t s = (hipStream_t)stream;
    double* d_edges = (double*)workspace;
    double* slots = d_edges + eo;
    u64* res = (u64*)d_result;
    OF3DK_HIP(hipMemsetAsync(d_result, 0, of3d_flow_pair_result_bytes(n_roi, nbins4), s));
    of3dk::put_edges(s, d_edges, host_edges, eo);
    const dim3 grid(max_nb, n_roi);
    auto launch = [&](auto vt) {
        using VT = decltype(vt);
        if (vz0)
            hipLaunchKernelGGL((k_pair_boxes<VT, false>), grid, dim3(kSumThreads), 0, s, (const VT*)vx0,
                               (const VT*)vy0, (const VT*)vz0, (const VT*)vx1, (const VT*)vy1, (const VT*)vz1, d_keep,
                               P, (const double*)d_edges, slots, res);
        else
            hipLaunchKernelGGL((k_pair_boxes<VT, true>), grid, dim3(kSumThreads), 0, s, (const VT*)vx0,
                               (const VT*)vy0, (const VT*)vz0, (const VT*)vx1, (const VT*)vy1, (const VT*)vz1, d_keep,
                               P, (const double*)d_edges, slots, res);
    };
    if (v_f32)
        launch(float{});
    else
        launch(double{});
    hipLaunchKernelGGL(k_pair_final, dim3(n_roi, kNSum / kGroup), dim3(of3dk::kFinalThreads), 0, s, (const double*)slots, P, res);
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// kt_whist.hip — magnitude-weighted histograms of the frame summary (of3d_flow_whist): per box
// and requested quantity np.histogram(values, bins=edges, weights=magnitude) over the valid
// voxels, the reference's distPhiW (plot_figure4_timeTraces.m:128-138: accumarray of the
// magnitudes over the discretized -phi).  A pass of its own over the fields, beside k_sum_boxes
// (kt_summary.hip) as k_proj_boxes (kt_axes.hip) is: the per-voxel arithmetic, the bin search,
// the walk and the workgroup partition are summary_dev.hpp's.
//   k_whist_boxes  one quantity per blockIdx.z; per wave a private LDS bin array, filled by a
//                  wave-uniform loop over the distinct bins among the lanes (no atomics)
//   k_whist_final  a thread per (box, quantity, bin): the workgroups' slots in index order
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "summary_dev.hpp"

namespace {

using u64 = unsigned long long;

using of3dk::kSumThreads, of3dk::kSumWaves, of3dk::kMaxBins, of3dk::kMaxRoi, of3dk::plan_boxes;  // summary_host.hpp
constexpr int kNQ = OF3D_SUMMARY_QUANTITIES;
constexpr size_t kEdgeWordsMax = (size_t)kNQ * (kMaxBins + 1);

// Requested quantities are numbered k = 0.. in QUANTITIES order; everything per quantity is
// indexed by k.  Workspace: the edges (eo words), then the slots [roi][k][workgroup][bin].
struct WhParams : of3dk::BoxParams {
    long long soff[kMaxRoi];  // first slot word of the box: sum over earlier boxes of nb * ntot
    int nq;                   // requested quantities
    int q[kNQ];               // the quantity (0 vx .. 5 phi)
    int nbins[kNQ];
    int eoff[kNQ];  // first edge in the workspace's edge array
    int hoff[kNQ];  // first bin among a box's bins
    int ntot;       // bins of a box, all quantities
    double sxy, sz, st;
};

__device__ __forceinline__ double readlane_f64(double v, int src) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((u64)b >> 32), src);
    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
}

// One voxel step of a wave: every lane holds a bin (-1: nothing to add) and a weight >= +0.0
// (0.0 with bin -1).  All 64 lanes call this together and run the same number of iterations:
// the loop condition is a ballot, so the shuffles inside see every lane.  Per distinct bin, in
// the order of its first lane: the weights of the lanes holding it (0.0 in the others, exact
// since weights are >= 0) added by the fixed shuffle tree of k_sum_boxes, then one plain
// read-modify-write of the wave's own array by lane 0.  A bin held by a single lane skips the
// tree: x + 0.0 == x bit for bit, so the tree would return that lane's weight unchanged.
__device__ __forceinline__ void wave_add(double* __restrict__ mine, int bin, double wgt, int lane) {
    u64 pending = __ballot(bin >= 0);
    while (pending) {
        const int leader = __ffsll(pending) - 1;
        const int b = __builtin_amdgcn_readlane(bin, leader);
        const bool match = bin == b;
        const u64 mm = __ballot(match);
        const double v = (mm & (mm - 1)) ? of3dk::wave_sum(match ? wgt : 0.0) : readlane_f64(wgt, leader);
        if (lane == 0) mine[b] += v;
        pending &= ~mm;
    }
}

// Grid (max workgroups of a box, n_roi, requested quantities).  Masked: the mask factor of a
// voxel is bit `roi` of keep (of3d_mask_open) instead of rel > thr.  The voxel loop and
// everything around wave_add is wave-uniform: invalid, out-of-range and tail lanes carry bin -1
// and weight 0.0 instead of leaving the loop.
template <typename VT, typename RelT, bool Masked>
__global__ __launch_bounds__(kSumThreads) void k_whist_boxes(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                             const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                             const RelT* __restrict__ thr_p,
                                                             const uint16_t* __restrict__ keep, WhParams P,
                                                             const double* __restrict__ edges_g,
                                                             double* __restrict__ slots, u64* __restrict__ result) {
    const int roi = blockIdx.y, nb = P.nb[roi], k = blockIdx.z;
    if ((int)blockIdx.x >= nb) return;
    __shared__ double edges[kMaxBins + 1];
    __shared__ double whist[kSumWaves][kMaxBins];
    __shared__ unsigned nvalid_s;
    const int q = P.q[k], nbins = P.nbins[k];
    for (int i = threadIdx.x; i <= nbins; i += kSumThreads) edges[i] = edges_g[P.eoff[k] + i];
    for (int i = threadIdx.x; i < kSumWaves * kMaxBins; i += kSumThreads) (&whist[0][0])[i] = 0.0;
    if (threadIdx.x == 0) nvalid_s = 0;
    __syncthreads();

    of3dk::BoxShare sh = of3dk::box_share(P, roi, nb);
    const of3dk::FlowFields<VT, RelT, Masked> F{vx,    vy,   vz,   rel, keep,         Masked ? 0.0 : (double)*thr_p,
                                                P.sxy, P.sz, P.st, roi, vz != nullptr};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* mine = whist[wave];
    unsigned nvalid = 0;

    of3dk::for_voxels_uniform(F, sh, [&](const of3dk::Voxel& vox, bool valid) {
        nvalid += valid;
        if (!__ballot(valid)) return;  // wave-uniform: no lane of this wave has anything to add
        const double mag = sqrt(vox.sq);
        const double v = of3dk::quantity_value(q, vox.vxp, vox.vyp, vox.vzp, mag, sqrt(vox.xy2));
        const int bin = valid ? of3dk::find_bin(edges, nbins, v) : -1;
        wave_add(mine, bin, bin >= 0 ? mag : 0.0, lane);
    });

    if (k == 0 && nvalid) atomicAdd(&nvalid_s, nvalid);
    __syncthreads();
    // the waves' arrays in wave order, into this workgroup's own slot
    double* slot = slots + P.soff[roi] + ((long long)nb * P.hoff[k] + (long long)blockIdx.x * nbins);
    for (int i = threadIdx.x; i < nbins; i += kSumThreads) {
        double v = whist[0][i];
        for (int j = 1; j < kSumWaves; ++j) v += whist[j][i];
        slot[i] = v;
    }
    if (threadIdx.x == 0 && nvalid_s) atomicAdd(&result[(size_t)roi * (1 + P.ntot)], (u64)nvalid_s);
}

// Grid (ceil(ntot / 256), n_roi): thread i of a box owns bin i of its bins and adds that bin's
// slots in workgroup-index order.
__global__ __launch_bounds__(256) void k_whist_final(const double* __restrict__ slots, WhParams P,
                                                     u64* __restrict__ result) {
    const int roi = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.ntot) return;
    int k = 0;
    while (k + 1 < P.nq && i >= P.hoff[k + 1]) ++k;
    const int nb = P.nb[roi], nbins = P.nbins[k];
    const double* s = slots + P.soff[roi] + ((long long)nb * P.hoff[k] + (i - P.hoff[k]));
    double v = s[0];
    for (int b = 1; b < nb; ++b) v += s[(size_t)b * nbins];
    result[(size_t)roi * (1 + P.ntot) + 1 + i] = (u64)__double_as_longlong(v);
}

}  // namespace

extern "C" {

size_t of3d_flow_whist_result_bytes(int n_roi, const int* nbins) {
    if (n_roi < 1 || n_roi > kMaxRoi || !of3dk::bins_ok<kNQ>(nbins)) return 0;
    return (size_t)n_roi * (1 + of3dk::total_bins<kNQ>(nbins)) * 8;
}

size_t of3d_flow_whist_workspace_bytes(const int64_t* rois, int n_roi, const int* nbins) {
    if (!of3dk::bins_ok<kNQ>(nbins)) {
        of3dk::set_error("of3d: 0 to 256 bins per quantity");
        return 0;
    }
    const int ntot = of3dk::total_bins<kNQ>(nbins);
    if (!ntot) {
        of3dk::set_error("of3d: a weighted histogram needs bins for at least one quantity");
        return 0;
    }
    size_t slot_words = 0;
    if (plan_boxes(rois, n_roi, nullptr, ntot, nullptr, nullptr, &slot_words) != 0) return 0;
    return (of3dk::edge_words<kNQ>(nbins) + slot_words) * sizeof(double);
}

int of3d_flow_whist(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                    int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                    double tscale, const int64_t* rois, int n_roi, const uint16_t* d_keep, const int* nbins,
                    const double* const* edges, void* d_result, void* workspace, void* stream) {
    if (!vx || !vy || !rois || !d_result || !workspace || (!d_keep && (!rel || !d_thresh)))
        return of3dk::set_error("of3d: null argument");
    if (of3dk::check_volume(nz, ny, nx, !vz) != 0) return -1;
    if (!of3dk::bins_ok<kNQ>(nbins)) return of3dk::set_error("of3d: 0 to 256 bins per quantity");
    if (!vz && (nbins[2] || nbins[5])) return of3dk::set_error("of3d: vz and phi histograms need a 3D volume");
    WhParams P{};
    P.sxy = xyscale, P.sz = zscale, P.st = tscale;
    P.ntot = of3dk::total_bins<kNQ>(nbins);
    if (!P.ntot) return of3dk::set_error("of3d: a weighted histogram needs bins for at least one quantity");
    const int64_t dims[3] = {nz, ny, nx};
    if (plan_boxes(rois, n_roi, dims, P.ntot, P.nb, P.soff) != 0) return -1;
    const int max_nb = of3dk::fill_boxes(P, dims, rois, n_roi);
    int all_nbins[kNQ], eoff[kNQ], hoff[kNQ];
    double host_edges[kEdgeWordsMax];
    const int eo = of3dk::plan_hists<kNQ>(nbins, edges, all_nbins, eoff, hoff, host_edges);
    if (eo < 0) return -1;
    for (int q = 0; q < kNQ; ++q) {  // the requested quantities, compacted
        if (!nbins[q]) continue;
        const int k = P.nq++;
        P.q[k] = q, P.nbins[k] = nbins[q], P.eoff[k] = eoff[q], P.hoff[k] = hoff[q];
    }
    hipStream_t s = (hipStream_t)stream;
    double* d_edges = (double*)workspace;
    double* slots = d_edges + eo;
    u64* res = (u64*)d_result;
    OF3DK_HIP(hipMemsetAsync(d_result, 0, of3d_flow_whist_result_bytes(n_roi, nbins), s));
    of3dk::put_edges(s, d_edges, host_edges, eo);
    const dim3 grid(max_nb, n_roi, P.nq);
    of3dk::with_flow_types(v_f32, rel_f64, d_keep != nullptr, [&](auto vt, auto rt, auto masked_c) {
        using VT = decltype(vt);
        using RT = decltype(rt);
        constexpr bool M = decltype(masked_c)::value;
        hipLaunchKernelGGL((k_whist_boxes<VT, RT, M>), grid, dim3(kSumThreads), 0, s, (const VT*)vx, (const VT*)vy,
                           (const VT*)vz, (const RT*)rel, (const RT*)d_thresh, d_keep, P, (const double*)d_edges, slots,
                           res);
    });
    hipLaunchKernelGGL(k_whist_final, dim3((P.ntot + 255) / 256, n_roi), dim3(256), 0, s, (const double*)slots, P, res);
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

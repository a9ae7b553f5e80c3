// kt_contract.hip — contractility of the flow with respect to the mask's centroid
// (of3d_flow_contract): what plot_figure2_movie.ipynb cell 1 of the reference does on the host
// with center_of_mass(relMask) and, per voxel, the angle between the velocity and the direction
// to that centre, here on the resident fields.
//   of3d_mask_axes  (kt_axes.hip, called without fields) the mask's exact integer sums n Sx Sy Sz
//   k_ct_centre     centroid = S / n, box-local, and the centre used, into the result
//   k_ct_boxes      k_sum_boxes' partition, masking and reduction (summary_dev.hpp) with the
//                   angle, its cosine and the inward speed in place of its eight quantities
//   k_ct_final      a box's workspace slots added in index order
// Stream-ordered end to end: k_ct_boxes reads the centre k_ct_centre left in the result; nothing
// returns to the host, no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "summary_dev.hpp"

namespace {

using u64 = unsigned long long;

using of3dk::kSumMaxBlocks, of3dk::kSumThreads, of3dk::kSumWaves, of3dk::kMaxBins, of3dk::kMaxRoi;  // summary_host.hpp

constexpr int kNQ = OF3D_CONTRACT_QUANTITIES;  // histograms: 0 angle (degrees), 1 inward
constexpr int kNSum = 4;                       // angle dot inward speed
// a box's result words (include/of3d.h)
constexpr int kWCentroid = 4, kWUsed = 7, kWValid = 10 /* then n_angle, n_inward */, kWSum = 13;
constexpr int kCtHead = OF3D_CONTRACT_ROI_WORDS;  // words before a box's histograms
constexpr size_t kEdgeWordsMax = (size_t)kNQ * (kMaxBins + 1);
// the moments' block of of3d_mask_axes (no histograms) at the head of the workspace
constexpr size_t kMomWords = (size_t)kMaxRoi * OF3D_AXES_ROI_WORDS;
constexpr double kDegrees = 180.0 / 3.14159265358979323846;  // np.degrees: x * (180 / pi)

// Workspace: of3d_mask_axes' result block, its workspace, the edges, the slots [roi][workgroup][4].
struct CtParams : of3dk::BoxParams {
    long long soff[kMaxRoi];  // first slot word of the box: sum over earlier boxes of nb * 4
    int nbins[kNQ];
    int eoff[kNQ];  // first edge of the quantity in the workspace's edge array
    int hoff[kNQ];  // first bin of the quantity in a box's histogram words
    int ntot;       // bins of a box, both quantities
    double sxy, sz, st;
};

struct GivenCentre {
    double c[3];  // x y z, box-local
    int use;
};

// One thread per box: the integers of3d_mask_axes left in `mom` into the result, the centroid
// as one float64 division of two integers exact in float64 (center_of_mass of an integer mask),
// and the centre k_ct_boxes measures from.
__global__ __launch_bounds__(64) void k_ct_centre(const u64* __restrict__ mom, GivenCentre given, int roi_words,
                                                  u64* __restrict__ result) {
    if (threadIdx.x != 0) return;
    const u64* m = mom + (size_t)blockIdx.x * OF3D_AXES_ROI_WORDS;
    u64* rr = result + (size_t)blockIdx.x * roi_words;
    const u64 n = m[0];
    for (int a = 0; a < 4; ++a) rr[a] = m[a];
    for (int a = 0; a < 3; ++a) {
        const double c = n ? (double)m[1 + a] / (double)n : __builtin_nan("");
        rr[kWCentroid + a] = (u64)__double_as_longlong(c);
        rr[kWUsed + a] = (u64)__double_as_longlong(given.use ? given.c[a] : c);
    }
}

// Grid (max workgroups of a box, n_roi).  Masked: the mask factor of a voxel is bit `roi` of
// keep (of3d_mask_open / of3d_mask_largest) instead of rel > thr.
template <typename VT, typename RelT, bool Masked>
__global__ __launch_bounds__(kSumThreads) void k_ct_boxes(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                          const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                          const RelT* __restrict__ thr_p,
                                                          const uint16_t* __restrict__ keep, CtParams P,
                                                          const double* __restrict__ edges_g,
                                                          double* __restrict__ slots, u64* __restrict__ result) {
    const int roi = blockIdx.y, nb = P.nb[roi];
    if ((int)blockIdx.x >= nb) return;
    __shared__ double edges[kEdgeWordsMax];
    __shared__ unsigned hist[kNQ * kMaxBins];
    __shared__ unsigned count_s[3];  // n_valid n_angle n_inward
    __shared__ double wsum[kSumWaves][kNSum];
    const int ne = (P.nbins[0] ? P.nbins[0] + 1 : 0) + (P.nbins[1] ? P.nbins[1] + 1 : 0);
    for (int i = threadIdx.x; i < ne; i += kSumThreads) edges[i] = edges_g[i];
    for (int i = threadIdx.x; i < P.ntot; i += kSumThreads) hist[i] = 0;
    if (threadIdx.x < 3) count_s[threadIdx.x] = 0;
    __syncthreads();

    u64* rr = result + (size_t)roi * (kCtHead + P.ntot);
    // the centre k_ct_centre left on this stream, in physical units: c.x*xyscale, c.y*xyscale, c.z*zscale
    const double cxs = __longlong_as_double((long long)rr[kWUsed + 0]) * P.sxy;
    const double cys = __longlong_as_double((long long)rr[kWUsed + 1]) * P.sxy;
    const double czs = __longlong_as_double((long long)rr[kWUsed + 2]) * P.sz;

    of3dk::BoxShare sh = of3dk::box_share(P, roi, nb);
    const of3dk::FlowFields<VT, RelT, Masked> F{vx,    vy,   vz,   rel, keep,         Masked ? 0.0 : (double)*thr_p,
                                                P.sxy, P.sz, P.st, roi, vz != nullptr};
    const bool is3 = F.is3;
    double acc[kNSum] = {0, 0, 0, 0};
    unsigned nvalid = 0, nangle = 0, ninward = 0;

    of3dk::for_valid_voxels(F, sh, [&](const of3dk::Voxel& v, unsigned kx, unsigned ky, unsigned kz) {
        const double vxp = v.vxp, vyp = v.vyp, vzp = v.vzp, speed = sqrt(v.sq);
        ++nvalid;
        // the notebook's expression trees, plain multiplies and adds in this order
        const double dx = (double)kx * P.sxy - cxs;
        const double dy = (double)ky * P.sxy - cys;
        const double dz = (double)kz * P.sz - czs;
        const double d2 = dx * dx + dy * dy;
        const double nd = is3 ? sqrt(d2 + dz * dz) : sqrt(d2);
        const double xy = (vxp / speed) * (-dx / nd) + (vyp / speed) * (-dy / nd);
        const double dot = is3 ? xy + (vzp / speed) * (-dz / nd) : xy;
        if (dot != dot) return;  // nd == 0 (the centre's own voxel) or no centre: no direction
        ++nangle;
        ninward += dot > 0.0;
        // stated deviation: numpy's arccos gives NaN a last bit beyond +-1, this gives 0 / 180
        const double angle = acos(fmin(fmax(dot, -1.0), 1.0)) * kDegrees;
        const double inward = speed * dot;
        acc[0] += angle;
        acc[1] += dot;
        acc[2] += inward;
        acc[3] += speed;
        if (P.nbins[0]) {
            const int b = of3dk::find_bin(edges + P.eoff[0], P.nbins[0], angle);
            if (b >= 0) atomicAdd(&hist[P.hoff[0] + b], 1u);
        }
        if (P.nbins[1]) {
            const int b = of3dk::find_bin(edges + P.eoff[1], P.nbins[1], inward);
            if (b >= 0) atomicAdd(&hist[P.hoff[1] + b], 1u);
        }
    });

    if (nvalid) atomicAdd(&count_s[0], nvalid);
    if (nangle) atomicAdd(&count_s[1], nangle);
    if (ninward) atomicAdd(&count_s[2], ninward);
    of3dk::reduce_to_slot(acc, wsum, slots + P.soff[roi] + (long long)blockIdx.x * kNSum);
    if (threadIdx.x < 3 && count_s[threadIdx.x]) atomicAdd(&rr[kWValid + threadIdx.x], (u64)count_s[threadIdx.x]);
    of3dk::flush_hist(hist, P.ntot, rr + kCtHead);
}

// One workgroup per box: its slots staged in LDS, then added in index order.
__global__ __launch_bounds__(of3dk::kFinalThreads) void k_ct_final(const double* __restrict__ slots, CtParams P,
                                                                   u64* __restrict__ result) {
    __shared__ double s[kSumMaxBlocks * kNSum];
    const int roi = blockIdx.x;
    of3dk::add_slots<kNSum, kNSum>(slots + P.soff[roi], P.nb[roi], s,
                                   result + (size_t)roi * (kCtHead + P.ntot) + kWSum);
}

}  // namespace

extern "C" {

size_t of3d_flow_contract_result_bytes(int n_roi, const int* nbins2) {
    if (n_roi < 1 || n_roi > kMaxRoi || !of3dk::bins_ok<kNQ>(nbins2)) return 0;
    return (size_t)n_roi * (kCtHead + of3dk::total_bins<kNQ>(nbins2)) * 8;
}

size_t of3d_flow_contract_workspace_bytes(const int64_t* rois, int n_roi, const int* nbins2) {
    if (!of3dk::bins_ok<kNQ>(nbins2)) {
        of3dk::set_error("of3d: 0 to 256 bins per quantity");
        return 0;
    }
    size_t slot_words = 0;
    if (of3dk::plan_boxes(rois, n_roi, nullptr, kNSum, nullptr, nullptr, &slot_words) != 0) return 0;
    const size_t mom_ws = of3d_mask_axes_workspace_bytes(rois, n_roi);  // 0: sums that could pass 2^63
    if (!mom_ws) return 0;
    return (kMomWords + of3dk::edge_words<kNQ>(nbins2) + slot_words) * 8 + mom_ws;
}

int of3d_flow_contract(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                       int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                       double tscale, const int64_t* rois, int n_roi, const uint16_t* d_keep,
                       const double* center_given, const int* nbins2, const double* const* edges2, void* d_result,
                       void* workspace, void* stream) {
    if (!vx || !vy || !rois || !d_result || !workspace || (!d_keep && (!rel || !d_thresh)))
        return of3dk::set_error("of3d: null argument");
    if (of3dk::check_volume(nz, ny, nx, !vz) != 0) return -1;
    if (vz && nz == 1) return of3dk::set_error("of3d: a 2D volume (nz == 1) takes no vz");
    if (!of3dk::bins_ok<kNQ>(nbins2)) return of3dk::set_error("of3d: 0 to 256 bins per quantity");
    CtParams P{};
    P.sxy = xyscale, P.sz = zscale, P.st = tscale;
    P.ntot = of3dk::total_bins<kNQ>(nbins2);
    const int64_t dims[3] = {nz, ny, nx};
    if (of3dk::plan_boxes(rois, n_roi, dims, kNSum, P.nb, P.soff) != 0) return -1;
    const int max_nb = of3dk::fill_boxes(P, dims, rois, n_roi);
    GivenCentre given;
    memset(&given, 0, sizeof(given));
    if (center_given) {
        for (int a = 0; a < 3; ++a) {
            if (!(center_given[a] - center_given[a] == 0.0))
                return of3dk::set_error("of3d: a given centre must be finite");
            given.c[a] = center_given[a];
        }
        given.use = 1;
    }
    double host_edges[kEdgeWordsMax];
    const int eo = of3dk::plan_hists<kNQ>(nbins2, edges2, P.nbins, P.eoff, P.hoff, host_edges);
    if (eo < 0) return -1;
    const size_t mom_ws = of3d_mask_axes_workspace_bytes(rois, n_roi);
    if (!mom_ws) return -1;
    hipStream_t s = (hipStream_t)stream;
    u64* mom = (u64*)workspace;
    char* axes_ws = (char*)(mom + kMomWords);
    double* d_edges = (double*)(axes_ws + mom_ws);
    double* slots = d_edges + eo;
    u64* res = (u64*)d_result;
    // the mask's integer sums: of3d_mask_axes' moment pass (steps 1-5, no fields)
    const int no_bins[OF3D_AXES_QUANTITIES] = {0, 0, 0};
    if (of3d_mask_axes(nullptr, nullptr, nullptr, rel, 0, rel_f64, nz, ny, nx, d_thresh, xyscale, zscale, tscale, rois,
                       n_roi, d_keep, nullptr, 0, no_bins, nullptr, mom, axes_ws, stream) != 0)
        return -1;
    OF3DK_HIP(hipMemsetAsync(d_result, 0, of3d_flow_contract_result_bytes(n_roi, nbins2), s));
    of3dk::put_edges(s, d_edges, host_edges, eo);
    hipLaunchKernelGGL(k_ct_centre, dim3(n_roi), dim3(64), 0, s, (const u64*)mom, given, kCtHead + P.ntot, res);
    const dim3 grid(max_nb, n_roi);
    of3dk::with_flow_types(v_f32, rel_f64, d_keep != nullptr, [&](auto vt, auto rt, auto masked_c) {
        using VT = decltype(vt);
        using RT = decltype(rt);
        constexpr bool M = decltype(masked_c)::value;
        hipLaunchKernelGGL((k_ct_boxes<VT, RT, M>), grid, dim3(kSumThreads), 0, s, (const VT*)vx, (const VT*)vy,
                           (const VT*)vz, (const RT*)rel, (const RT*)d_thresh, d_keep, P, (const double*)d_edges, slots,
                           res);
    });
    hipLaunchKernelGGL(k_ct_final, dim3(n_roi), dim3(of3dk::kFinalThreads), 0, s, (const double*)slots, P, res);
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// kt_axes.hip — the body-axis frame of a reliability mask and the flow projected onto it
// (of3d_mask_axes): what plot_figure5.m:87-88,132-149 and plot_figure5_Movie.m:88-89,128-143 of
// the reference do on the host with regionprops3(relMask, 'EigenVectors', 'EigenValues') and a
// projection of every velocity vector onto the first eigenvectors, here on the resident fields.
//   k_mom_boxes   integer moments of the mask over box-local coordinates (no floating point)
//   k_axes        centroid, exact central moments (128-bit integers), covariance, Jacobi
//   k_proj_boxes  k_sum_boxes' per-voxel arithmetic, projected on the axes: sums and histograms
//   k_proj_final  a box's workspace slots added in index order
// Stream-ordered end to end: nothing returns to the host, no workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "summary_dev.hpp"

namespace {

using u32 = unsigned;
using u64 = unsigned long long;
using u128 = unsigned __int128;
using i128 = __int128;

using of3dk::kSumMaxBlocks, of3dk::kSumThreads, of3dk::kSumWaves, of3dk::kMaxBins, of3dk::kMaxRoi;  // summary_host.hpp

constexpr int kNA = OF3D_AXES_QUANTITIES;  // projections (axes)
constexpr int kNMom = 10;                  // n x y z xx yy zz xy xz yz
// a box's result words (include/of3d.h)
constexpr int kWCentroid = 10, kWCov = 13, kWVal = 19, kWVec = 22, kWUsed = 31, kWValid = 40, kWSum = 41;
constexpr int kAxHead = OF3D_AXES_ROI_WORDS;  // words before a box's histograms
// The moment pass ends in ten same-line atomics per workgroup, which the memory side takes one
// after another: few, large workgroups (16 waves; at most two per compute unit of an MI355X).
constexpr int kMomThreads = 1024, kMomWaves = kMomThreads / 64;
constexpr int kMomMaxBlocks = 512;  // workgroups of the moment pass per box at most
constexpr int kMomUnroll = 4;        // segments of a row a wave has in flight
constexpr int kSweeps = 12;          // cyclic Jacobi sweeps (a 3x3 is converged after 5 or 6)
constexpr size_t kAxSlotBytes = (size_t)kMaxRoi * kSumMaxBlocks * kNA * sizeof(double);
constexpr size_t kAxEdgeWords = (size_t)kNA * (kMaxBins + 1);
constexpr size_t kAxWsBytes = kAxSlotBytes + kAxEdgeWords * sizeof(double);

struct AxParams : of3dk::BoxParams {  // nb: the workgroups of the box in k_proj_boxes, 0 without a projection
    int nbins[kNA];
    int eoff[kNA];  // first edge of the axis in the workspace's edge array
    int hoff[kNA];  // first bin of the axis in a box's histogram words
    int roi_words;  // result words per box
    int physical;   // covariance in physical units (S C S) before the eigen-decomposition
    double sxy, sz, st;
};

struct GivenAxes {
    double a[9];  // e1 e2 e3, each x y z
    int use;
};

// ---------------------------------------------------------------------------
// Moments.  Wave w of the grid takes the rows (z, y) w, w + W, ... of the box (W waves in all)
// and walks a row in segments of 64 x; lane l of segment s holds x = 64*s + l.  With m the
// lane's mask bit and c = popcount(ballot(m)) of a segment,
//   sum m*x   = 64 * sum_s s*c + sum_l l * n_l                      n_l = sum m    of lane l
//   sum m*x^2 = 4096 * sum_s s^2*c + 128 * sum_l l * p_l + sum_l l^2 * n_l   p_l = sum m*s
//   sum m*x*y = y * (the row's sum m*x): 64 * y * sum_s s*c + sum_l l * q_l  q_l = sum m*y
// and likewise z.  So a segment costs one ballot, a popcount and two wave-uniform
// multiply-adds, and four per-lane accumulators (n_l, p_l, q_l for y and for z); y, z and
// their squares multiply a row's totals once per row, and the lane index once at the end.
// Integers throughout: exact and independent of the order.
// ---------------------------------------------------------------------------
__device__ __forceinline__ u64 mul32(u32 a, u32 b) { return (u64)a * (u64)b; }

template <typename RelT, bool Masked>
__global__ __launch_bounds__(kMomThreads) void k_mom_boxes(const RelT* __restrict__ rel,
                                                           const RelT* __restrict__ thr_p,
                                                           const uint16_t* __restrict__ keep, AxParams P,
                                                           u64* __restrict__ result) {
    __shared__ u64 part[kMomWaves][kNMom];
    const int roi = blockIdx.y;
    const u32 lane = threadIdx.x & 63;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int z0 = P.box[roi][0], y0 = P.box[roi][2], x0 = P.box[roi][4];
    const u32 dy = P.box[roi][3] - y0, dx = P.box[roi][5] - x0;
    const u32 nseg = (dx + 63) / 64;
    const u64 rows = (u64)(P.box[roi][1] - z0) * dy;
    const u32 W = gridDim.x * kMomWaves;
    // this wave's row as (z, y), advanced by W rows per step without divisions
    u64 row = (u64)blockIdx.x * kMomWaves + wave;
    const u32 step_y = W % dy, step_z = W / dy;
    u32 y = (u32)(row % dy), z = (u32)(row / dy);
    RelT thr = (RelT)0;
    if constexpr (!Masked) thr = *thr_p;

    u64 s_n = 0, s_y = 0, s_z = 0, s_yy = 0, s_zz = 0, s_yz = 0;  // wave-uniform
    u64 s_t1 = 0, s_t2 = 0, s_t1y = 0, s_t1z = 0;                 // sum s*c, s^2*c, y*s*c, z*s*c
    u32 n_l = 0;                                                  // per lane
    u64 p_l = 0, qy_l = 0, qz_l = 0;
    for (; row < rows; row += W) {
        const size_t base = ((size_t)(z0 + z) * P.ny + (y0 + y)) * P.nx + x0;
        u64 c_row = 0, t1 = 0, t2 = 0;  // the row's sum c, s*c, s^2*c
        u32 nl_row = 0;                 // this lane's mask voxels of the row
        for (u32 s0 = 0; s0 < nseg; s0 += kMomUnroll) {
            bool m[kMomUnroll];
#pragma unroll
            for (int u = 0; u < kMomUnroll; ++u) {
                const u32 x = (s0 + u) * 64 + lane;
                m[u] = false;
                if (x < dx) {  // also false for a segment past the row: x >= 64 * nseg >= dx
                    if constexpr (Masked)
                        m[u] = keep[base + x] >> roi & 1;
                    else
                        m[u] = rel[base + x] > thr;  // NaN on either side: false
                }
            }
#pragma unroll
            for (int u = 0; u < kMomUnroll; ++u) {
                const u32 sg = s0 + u;
                const u32 c = (u32)__popcll(__ballot(m[u]));
                const u64 sc = mul32(sg, c);  // s < 2^25, c <= 64
                c_row += c;
                t1 += sc;
                t2 += sc * sg;  // < 2^56
                nl_row += m[u];
                p_l += m[u] ? sg : 0u;
            }
        }
        n_l += nl_row;
        qy_l += mul32(nl_row, y);
        qz_l += mul32(nl_row, z);
        const u64 yy = mul32(y, y), zz = mul32(z, z), yz = mul32(y, z);
        s_n += c_row;
        s_y += c_row * y;
        s_z += c_row * z;
        s_yy += c_row * yy;
        s_zz += c_row * zz;
        s_yz += c_row * yz;
        s_t1 += t1;
        s_t2 += t2;
        s_t1y += t1 * y;
        s_t1z += t1 * z;
        y += step_y;
        const u32 carry = y >= dy;
        y -= carry ? dy : 0;
        z += step_z + carry;
    }
    // the lane index enters once: sum_l l*n_l, l*p_l, l^2*n_l, l*q_l
    u64 lx = (u64)lane * n_l, lxx = 128 * (u64)lane * p_l + (u64)(lane * lane) * n_l;
    u64 lxy = (u64)lane * qy_l, lxz = (u64)lane * qz_l;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lx += __shfl_down(lx, off, 64);
        lxx += __shfl_down(lxx, off, 64);
        lxy += __shfl_down(lxy, off, 64);
        lxz += __shfl_down(lxz, off, 64);
    }
    if (lane == 0) {
        u64* p = part[wave];
        p[0] = s_n, p[1] = 64 * s_t1 + lx, p[2] = s_y, p[3] = s_z, p[4] = 4096 * s_t2 + lxx, p[5] = s_yy, p[6] = s_zz;
        p[7] = 64 * s_t1y + lxy, p[8] = 64 * s_t1z + lxz, p[9] = s_yz;
    }
    __syncthreads();
    if (threadIdx.x < kNMom) {
        u64 v = 0;
        for (int w = 0; w < kMomWaves; ++w) v += part[w][threadIdx.x];
        if (v) atomicAdd(&result[(size_t)roi * P.roi_words + threadIdx.x], v);
    }
}

// ---------------------------------------------------------------------------
// Axes.  n*S_ab - S_a*S_b exactly in 128-bit integers, then fp64.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double to_double(u128 v) {
    return (double)(u64)(v >> 64) * 18446744073709551616.0 + (double)(u64)v;
}

// (n*sab - sa*sb) / n^2: the population central moment
__device__ __forceinline__ double central(u64 n, u64 sab, u64 sa, u64 sb) {
    const i128 d = (i128)((u128)n * sab) - (i128)((u128)sa * sb);
    const double mag = to_double(d < 0 ? (u128)(-d) : (u128)d);
    const double v = mag / ((double)n * (double)n);
    return d < 0 ? -v : v;
}

// one Jacobi rotation annihilating a[p][q] (Rutishauser's formulas); v's columns are the vectors
__device__ __forceinline__ void rotate(double a[3][3], double v[3][3], int p, int q) {
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const int r = 3 - p - q;  // the third index
    a[p][p] = a[p][p] - t * apq;
    a[q][q] = a[q][q] + t * apq;
    a[p][q] = a[q][p] = 0.0;
    const double arp = a[r][p], arq = a[r][q];
    a[r][p] = a[p][r] = c * arp - s * arq;
    a[r][q] = a[q][r] = s * arp + c * arq;
    for (int k = 0; k < 3; ++k) {
        const double vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
    }
}

__global__ __launch_bounds__(64) void k_axes(AxParams P, GivenAxes given, u64* __restrict__ result) {
    if (threadIdx.x != 0) return;
    const int roi = blockIdx.x;
    u64* rr = result + (size_t)roi * P.roi_words;
    auto put = [&](int w, double v) { rr[w] = (u64)__double_as_longlong(v); };
    const u64 n = rr[0];
    if (given.use)
        for (int i = 0; i < 9; ++i) put(kWUsed + i, given.a[i]);
    if (n == 0) {
        const double qnan = __builtin_nan("");
        for (int w = kWCentroid; w < (given.use ? kWUsed : kWValid); ++w) put(w, qnan);
        return;
    }
    const u64 sx = rr[1], sy = rr[2], sz = rr[3];
    const double dn = (double)n;
    put(kWCentroid + 0, (double)P.box[roi][4] + (double)sx / dn);
    put(kWCentroid + 1, (double)P.box[roi][2] + (double)sy / dn);
    put(kWCentroid + 2, (double)P.box[roi][0] + (double)sz / dn);
    double a[3][3], v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    a[0][0] = central(n, rr[4], sx, sx);
    a[1][1] = central(n, rr[5], sy, sy);
    a[2][2] = central(n, rr[6], sz, sz);
    a[0][1] = a[1][0] = central(n, rr[7], sx, sy);
    a[0][2] = a[2][0] = central(n, rr[8], sx, sz);
    a[1][2] = a[2][1] = central(n, rr[9], sy, sz);
    if (P.physical) {
        const double s[3] = {P.sxy, P.sxy, P.sz};
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j) a[i][j] = a[j][i] = (s[i] * a[i][j]) * s[j];  // one rounding order: symmetric
    }
    put(kWCov + 0, a[0][0]), put(kWCov + 1, a[1][1]), put(kWCov + 2, a[2][2]);
    put(kWCov + 3, a[0][1]), put(kWCov + 4, a[0][2]), put(kWCov + 5, a[1][2]);
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        rotate(a, v, 0, 1);
        rotate(a, v, 0, 2);
        rotate(a, v, 1, 2);
    }
    // a covariance has no negative eigenvalue: one that rounding left below zero is zero
    double lam[3];
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 3; ++i) lam[i] = a[i][i] < 0.0 ? 0.0 : a[i][i];
    // descending, stable (equal values keep the x, y, z order): three compare-exchanges
    auto cx = [&](int i, int j) {
        if (lam[ord[j]] > lam[ord[i]]) {
            const int t = ord[i];
            ord[i] = ord[j], ord[j] = t;
        }
    };
    cx(0, 1), cx(1, 2), cx(0, 1);
    for (int k = 0; k < 3; ++k) {
        const int c = ord[k];
        double e[3] = {v[0][c], v[1][c], v[2][c]};
        // sign: the component of largest magnitude is positive, a tie goes to the first
        int big = 0;
        for (int i = 1; i < 3; ++i)
            if (fabs(e[i]) > fabs(e[big])) big = i;
        const bool flip = e[big] < 0.0;
        put(kWVal + k, lam[c]);
        for (int i = 0; i < 3; ++i) {
            const double ei = flip ? -e[i] : e[i];
            put(kWVec + 3 * k + i, ei);
            if (!given.use) put(kWUsed + 3 * k + i, ei);
        }
    }
}

// ---------------------------------------------------------------------------
// Projection.  k_sum_boxes' partition, masking and reduction (summary_dev.hpp, kt_summary.hip)
// with p_k = (vx*e_k.x + vy*e_k.y) + vz*e_k.z in place of its eight quantities.
// ---------------------------------------------------------------------------
template <typename VT, typename RelT, bool Masked>
__global__ __launch_bounds__(kSumThreads) void k_proj_boxes(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                            const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                            const RelT* __restrict__ thr_p,
                                                            const uint16_t* __restrict__ keep, AxParams P,
                                                            const double* __restrict__ edges_g,
                                                            double* __restrict__ slots, u64* __restrict__ result) {
    const int roi = blockIdx.y, nb = P.nb[roi];
    if ((int)blockIdx.x >= nb) return;
    __shared__ double edges[kAxEdgeWords];
    __shared__ unsigned hist[kNA * kMaxBins];
    __shared__ unsigned nvalid_s;
    __shared__ double wsum[kSumWaves][kNA];
    int ntot = 0, ne = 0;
    for (int q = 0; q < kNA; ++q) {
        ntot += P.nbins[q];
        ne += P.nbins[q] ? P.nbins[q] + 1 : 0;
    }
    for (int i = threadIdx.x; i < ne; i += kSumThreads) edges[i] = edges_g[i];
    for (int i = threadIdx.x; i < ntot; i += kSumThreads) hist[i] = 0;
    if (threadIdx.x == 0) nvalid_s = 0;
    __syncthreads();

    u64* rr = result + (size_t)roi * P.roi_words;
    double ax[kNA][3];  // the axes k_axes left on this stream
#pragma unroll
    for (int k = 0; k < kNA; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i) ax[k][i] = __longlong_as_double((long long)rr[kWUsed + 3 * k + i]);

    of3dk::BoxShare sh = of3dk::box_share(P, roi, nb);
    const of3dk::FlowFields<VT, RelT, Masked> F{vx,    vy,   vz,   rel, keep,         Masked ? 0.0 : (double)*thr_p,
                                                P.sxy, P.sz, P.st, roi, vz != nullptr};
    const bool is3 = F.is3;
    double acc[kNA] = {0, 0, 0};
    unsigned nvalid = 0;

    // no root is taken: the sum of squares says whether the voxel is valid
    of3dk::for_valid_voxels(F, sh, [&](const of3dk::Voxel& v, unsigned, unsigned, unsigned) {
        ++nvalid;
#pragma unroll
        for (int k = 0; k < kNA; ++k) {
            const double xy = v.vxp * ax[k][0] + v.vyp * ax[k][1];
            const double p = is3 ? xy + v.vzp * ax[k][2] : xy;
            acc[k] += p;
            if (P.nbins[k]) {
                const int b = of3dk::find_bin(edges + P.eoff[k], P.nbins[k], p);
                if (b >= 0) atomicAdd(&hist[P.hoff[k] + b], 1u);
            }
        }
    });

    if (nvalid) atomicAdd(&nvalid_s, nvalid);
    of3dk::reduce_to_slot(acc, wsum, slots + ((size_t)roi * kSumMaxBlocks + blockIdx.x) * kNA);
    if (threadIdx.x == 0 && nvalid_s) atomicAdd(&rr[kWValid], (u64)nvalid_s);
    of3dk::flush_hist(hist, ntot, rr + kAxHead);
}

// One workgroup per box: its slots staged in LDS, then added in index order.
__global__ __launch_bounds__(of3dk::kFinalThreads) void k_proj_final(const double* __restrict__ slots, AxParams P,
                                                                     u64* __restrict__ result) {
    __shared__ double s[kSumMaxBlocks * kNA];
    const int roi = blockIdx.x;
    of3dk::add_slots<kNA, kNA>(slots + (size_t)roi * kSumMaxBlocks * kNA, P.nb[roi], s,
                               result + (size_t)roi * P.roi_words + kWSum);
}

int roi_words(const int* nbins3) { return kAxHead + of3dk::total_bins<kNA>(nbins3); }

// The boxes as of3d_flow_summary validates them, and the moments' range: the largest sum is
// sum a^2 <= voxels * (L - 1)^2 with L the box's longest edge, which must stay below 2^63.
int check_boxes(const int64_t* rois, int n_roi, const int64_t dims[3]) {
    if (of3dk::check_roi_count(rois, n_roi) != 0) return -1;
    for (int r = 0; r < n_roi; ++r) {
        u128 vox = 1;
        int64_t longest = 0;
        for (int a = 0; a < 3; ++a) {
            const int64_t ext = of3dk::box_extent(rois, r, a, dims);
            if (ext < 0) return -1;
            vox *= (u128)ext;
            longest = ext > longest ? ext : longest;
        }
        // vox < 2^93 and (L - 1)^2 < 2^62: the first test keeps the product inside 128 bits
        if (vox >= ((u128)1 << 63) || vox * (u128)(longest - 1) * (u128)(longest - 1) >= ((u128)1 << 63))
            return of3dk::set_error(("of3d: ROI " + std::to_string(r) + " is too large for 64-bit moments").c_str());
    }
    return 0;
}

}  // namespace

extern "C" {

size_t of3d_mask_axes_workspace_bytes(const int64_t* rois, int n_roi) {
    return check_boxes(rois, n_roi, nullptr) == 0 ? kAxWsBytes : 0;
}

size_t of3d_mask_axes_result_bytes(int n_roi, const int* nbins3) {
    if (n_roi < 1 || n_roi > kMaxRoi || !of3dk::bins_ok<kNA>(nbins3)) return 0;
    return (size_t)n_roi * roi_words(nbins3) * 8;
}

int of3d_mask_axes(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64, int64_t nz,
                   int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale, double tscale,
                   const int64_t* rois, int n_roi, const uint16_t* d_keep, const double* axes_given,
                   int axes_physical, const int* nbins3, const double* const* edges3, void* d_result,
                   void* workspace, void* stream) {
    const bool project = vx != nullptr;  // no fields: the mask's part alone
    if (!rois || !d_result || !workspace || (!d_keep && (!rel || !d_thresh)) || (project && !vy) ||
        (!project && (vy || vz)))
        return of3dk::set_error("of3d: null argument");
    if (of3dk::check_volume(nz, ny, nx, project && !vz) != 0) return -1;
    if (!of3dk::bins_ok<kNA>(nbins3)) return of3dk::set_error("of3d: 0 to 256 bins per quantity");
    if (!project && (nbins3[0] || nbins3[1] || nbins3[2]))
        return of3dk::set_error("of3d: axis histograms need the velocity fields");
    if (project && !vz && nbins3[2]) return of3dk::set_error("of3d: an axis3 histogram needs a 3D volume");
    const int64_t dims[3] = {nz, ny, nx};
    if (check_boxes(rois, n_roi, dims) != 0) return -1;
    GivenAxes given;
    memset(&given, 0, sizeof(given));
    if (axes_given) {
        for (int i = 0; i < 9; ++i) {
            if (!(axes_given[i] - axes_given[i] == 0.0)) return of3dk::set_error("of3d: given axes must be finite");
            given.a[i] = axes_given[i];
        }
        given.use = 1;
    }
    AxParams P{};
    P.sxy = xyscale, P.sz = zscale, P.st = tscale, P.physical = axes_physical != 0;
    if (project && of3dk::plan_boxes(rois, n_roi, dims, 0, P.nb) != 0) return -1;
    const int max_nb = of3dk::fill_boxes(P, dims, rois, n_roi);
    unsigned max_mom = 1;
    for (int r = 0; r < n_roi; ++r) {
        // the moment pass: a row per wave and step
        const int64_t rows = (rois[r * 6 + 1] - rois[r * 6]) * (rois[r * 6 + 3] - rois[r * 6 + 2]);
        const int64_t want = (rows + kMomWaves - 1) / kMomWaves;
        const unsigned mb = (unsigned)(want > kMomMaxBlocks ? kMomMaxBlocks : want);
        max_mom = mb > max_mom ? mb : max_mom;
    }
    double host_edges[kAxEdgeWords];
    const int eo = of3dk::plan_hists<kNA>(nbins3, edges3, P.nbins, P.eoff, P.hoff, host_edges);
    if (eo < 0) return -1;
    P.roi_words = roi_words(nbins3);
    hipStream_t s = (hipStream_t)stream;
    double* slots = (double*)workspace;
    double* d_edges = (double*)((char*)workspace + kAxSlotBytes);
    u64* res = (u64*)d_result;
    OF3DK_HIP(hipMemsetAsync(d_result, 0, of3d_mask_axes_result_bytes(n_roi, nbins3), s));
    of3dk::put_edges(s, d_edges, host_edges, eo);
    const dim3 mgrid(max_mom, n_roi), mblock(kMomThreads);
    if (d_keep)
        hipLaunchKernelGGL((k_mom_boxes<float, true>), mgrid, mblock, 0, s, (const float*)nullptr,
                           (const float*)nullptr, d_keep, P, res);
    else if (rel_f64)
        hipLaunchKernelGGL((k_mom_boxes<double, false>), mgrid, mblock, 0, s, (const double*)rel,
                           (const double*)d_thresh, d_keep, P, res);
    else
        hipLaunchKernelGGL((k_mom_boxes<float, false>), mgrid, mblock, 0, s, (const float*)rel,
                           (const float*)d_thresh, d_keep, P, res);
    hipLaunchKernelGGL(k_axes, dim3(n_roi), dim3(64), 0, s, P, given, res);
    if (project)
        of3dk::with_flow_types(v_f32, rel_f64, d_keep != nullptr, [&](auto vt, auto rt, auto masked_c) {
            using VT = decltype(vt);
            using RT = decltype(rt);
            constexpr bool M = decltype(masked_c)::value;
            hipLaunchKernelGGL((k_proj_boxes<VT, RT, M>), dim3(max_nb, n_roi), dim3(kSumThreads), 0, s, (const VT*)vx,
                               (const VT*)vy, (const VT*)vz, (const RT*)rel, (const RT*)d_thresh, d_keep, P,
                               (const double*)d_edges, slots, res);
            hipLaunchKernelGGL(k_proj_final, dim3(n_roi), dim3(of3dk::kFinalThreads), 0, s, (const double*)slots, P,
                               res);
        });
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

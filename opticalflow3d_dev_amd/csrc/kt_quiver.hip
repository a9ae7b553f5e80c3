// kt_quiver.hip — quiver samples of the frame summary (of3d_quiver_sample): per box the voxels of
// the gap lattice anchored at the box origin whose masked velocity is not NaN, in C order, as
// (linear index, vx, vy, vz) records — what the reference's figure scripts hand to quiver /
// quiver3 (example_analysis_script.m:64-66,121-135, plot_figure4_Movies.m:121-143: y1:gap:y2
// of the ROI, ~isnan of the masked velocity).  An ordered stream compaction in three
// stream-ordered launches, none of whose workgroups waits for another:
//   k_quiver_count  a wave per contiguous sub-run of a workgroup's lattice rows: its valid count
//   k_quiver_scan   a workgroup per box: the exclusive scan of the wave counts, and the header
//   k_quiver_emit   the walk of k_quiver_count again; lane position = base + lanes below
// The walk and the predicate are one function (walk_wave) for both passes; the per-voxel
// arithmetic, the walk over a box and the workgroup partition are summary_dev.hpp's, here over
// the lattice's extents.  No atomics of any kind: every record's slot is a function of the
// inputs alone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "summary_dev.hpp"

namespace {

using u64 = unsigned long long;

using of3dk::kSumThreads, of3dk::kSumWaves, of3dk::kMaxRoi, of3dk::kSumMaxBlocks;  // summary_host.hpp
constexpr int kHead = OF3D_QUIVER_HEAD_WORDS, kRoiHead = OF3D_QUIVER_ROI_WORDS;

// `box` holds the boxes in the volume, nb the workgroups of a box's LATTICE (plan_boxes over the
// lattice extents).  Workspace: one word per wave of every workgroup, [roi][workgroup][wave].
struct QvParams : of3dk::BoxParams {
    int gap[3];                // gz gy gx (a gap beyond 2^31 - 1 acts as 2^31 - 1: one point on that axis)
    int lat[kMaxRoi][3];       // lattice extents lz ly lx of the box: ceil(extent / gap)
    long long woff[kMaxRoi];   // first workspace word of the box
    long long boff[kMaxRoi];   // first result word of the box's block
    long long cap[kMaxRoi];    // records the block holds
    double sxy, sz, st;
};

// Wave `wave` of workgroup blockIdx.x of box `roi`: its sub-run of the workgroup's lattice points,
// 64 consecutive points per step.  Returns the number of valid points (the same in every lane).
// Emit: the valid point of a lane is record base + (valid lanes below it) of the box, stored
// where that is below the capacity.  Everything around the ballot is wave-uniform.
template <typename VT, typename RelT, bool Masked, bool Emit>
__device__ __forceinline__ u64 walk_wave(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                         const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                         const RelT* __restrict__ thr_p, const uint16_t* __restrict__ keep,
                                         const QvParams& P, int roi, u64 base, u64* __restrict__ block) {
    const int nb = P.nb[roi], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned ly = P.lat[roi][1], lx = P.lat[roi][2];
    const long long R = (long long)P.lat[roi][0] * ly;
    const long long r0 = R * blockIdx.x / nb, r1 = R * (blockIdx.x + 1) / nb;
    const long long count = (r1 - r0) * lx;  // this workgroup's points (< 2^31: checked on the host)
    const long long p0 = count * wave / kSumWaves, p1 = count * (wave + 1) / kSumWaves;
    of3dk::BoxWalk w(ly, lx, r0, (unsigned)(p0 + lane), 64);
    const int z0 = P.box[roi][0], y0 = P.box[roi][2], x0 = P.box[roi][4];
    const size_t ny = P.ny, nx = P.nx;
    const of3dk::FlowFields<VT, RelT, Masked> F{vx,    vy,   vz,   rel, keep,         Masked ? 0.0 : (double)*thr_p,
                                                P.sxy, P.sz, P.st, roi, vz != nullptr};
    const long long cap = P.cap[roi];
    const u64 below = ((u64)1 << lane) - 1;
    u64 n = 0;
    for (long long e = p0; e < p1; e += 64) {  // the same trips in every lane
        if (Emit && (long long)(base + n) >= cap) break;  // wave-uniform: the block is full
        of3dk::RawVoxel raw{0.0, 0.0, 0.0, 0.0};  // past the end: mask factor 0, not valid
        size_t i = 0;
        if (e + lane < p1) {
            i = ((size_t)(z0 + (size_t)w.z * P.gap[0]) * ny + (y0 + (size_t)w.y * P.gap[1])) * nx +
                (x0 + (size_t)w.x * P.gap[2]);
            raw = of3dk::load_voxel(F, i);
        }
        w.advance();
        const of3dk::Voxel v = of3dk::physical_voxel(F, raw);
        const double vxp = v.vxp, vyp = v.vyp, vzp = v.vzp;
        const bool valid = v.sq == v.sq;
        const u64 bal = __ballot(valid);
        if constexpr (Emit) {
            const long long pos = (long long)(base + n) + __popcll(bal & below);
            if (valid && pos < cap) {
                block[pos] = (u64)i;
                block[cap + pos] = (u64)__double_as_longlong(vxp);
                block[2 * cap + pos] = (u64)__double_as_longlong(vyp);
                block[3 * cap + pos] = (u64)__double_as_longlong(vzp);
            }
        }
        n += __popcll(bal);
    }
    return n;
}

// Grid (max workgroups of a box, n_roi).  Masked: the mask factor of a voxel is bit `roi` of keep
// (of3d_mask_open) instead of rel > thr.
template <typename VT, typename RelT, bool Masked>
__global__ __launch_bounds__(kSumThreads) void k_quiver_count(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                              const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                              const RelT* __restrict__ thr_p,
                                                              const uint16_t* __restrict__ keep, QvParams P,
                                                              u64* __restrict__ ws) {
    const int roi = blockIdx.y;
    if ((int)blockIdx.x >= P.nb[roi]) return;
    const u64 n = walk_wave<VT, RelT, Masked, false>(vx, vy, vz, rel, thr_p, keep, P, roi, 0, nullptr);
    if ((threadIdx.x & 63) == 0) ws[P.woff[roi] + (long long)blockIdx.x * kSumWaves + (threadIdx.x >> 6)] = n;
}

// Grid (n_roi), kSumMaxBlocks threads: thread t owns workgroup t of the box.  Its waves' counts
// become their exclusive prefix over the whole box (the order of the records: workgroup, then
// wave), by a shuffle scan over each wave's lanes and the waves' totals in LDS.
constexpr int kScanThreads = kSumMaxBlocks, kScanWaves = kScanThreads / 64;
__global__ __launch_bounds__(kScanThreads) void k_quiver_scan(u64* __restrict__ ws, QvParams P, const void* thr_p,
                                                              int rel_f64, long long gz, long long gy, long long gx,
                                                              int has_vz, u64* __restrict__ result) {
    const int roi = blockIdx.x, nb = P.nb[roi], t = threadIdx.x, lane = t & 63, wave = t >> 6;
    __shared__ u64 wtot[kScanWaves];
    u64* mine = ws + P.woff[roi] + (long long)t * kSumWaves;
    u64 c[kSumWaves], own = 0;
#pragma unroll
    for (int j = 0; j < kSumWaves; ++j) {
        c[j] = t < nb ? mine[j] : 0;
        own += c[j];
    }
    u64 incl = own;  // inclusive scan over the wave's lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    u64 before = 0, total = 0;
    for (int j = 0; j < kScanWaves; ++j) {
        before += j < wave ? wtot[j] : 0;
        total += wtot[j];
    }
    u64 base = before + incl - own;
    if (t < nb) {
#pragma unroll
        for (int j = 0; j < kSumWaves; ++j) {
            mine[j] = base;
            base += c[j];
        }
    }
    if (t == 0) {
        u64* h = result + kHead + (size_t)roi * kRoiHead;
        const u64 cap = (u64)P.cap[roi];
        h[0] = (u64)P.lat[roi][0] * (u64)P.lat[roi][1] * (u64)P.lat[roi][2];
        h[1] = total;
        h[2] = total < cap ? total : cap;
        h[3] = (u64)P.boff[roi];
        if (roi == 0) {
            double thr = __builtin_nan("");
            if (thr_p) thr = rel_f64 ? *(const double*)thr_p : (double)*(const float*)thr_p;
            result[0] = (u64)__double_as_longlong(thr);
            result[1] = (u64)P.n_roi;
            result[2] = (u64)gz, result[3] = (u64)gy, result[4] = (u64)gx;
            result[5] = (u64)has_vz;
        }
    }
}

template <typename VT, typename RelT, bool Masked>
__global__ __launch_bounds__(kSumThreads) void k_quiver_emit(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                             const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                             const RelT* __restrict__ thr_p,
                                                             const uint16_t* __restrict__ keep, QvParams P,
                                                             const u64* __restrict__ ws, u64* __restrict__ result) {
    const int roi = blockIdx.y;
    if ((int)blockIdx.x >= P.nb[roi]) return;
    const u64 base = ws[P.woff[roi] + (long long)blockIdx.x * kSumWaves + (threadIdx.x >> 6)];
    walk_wave<VT, RelT, Masked, true>(vx, vy, vz, rel, thr_p, keep, P, roi, base, result + P.boff[roi]);
}

// The capacities checked and summed: the result's words, 0 with the error set
size_t result_words(int n_roi, const int64_t* capacity) {
    if (!capacity) return of3dk::set_error("of3d: null argument"), 0;
    if (n_roi < 1 || n_roi > kMaxRoi) return of3dk::set_error("of3d: 1 to 16 ROI boxes"), 0;
    size_t words = kHead + (size_t)n_roi * kRoiHead;
    for (int r = 0; r < n_roi; ++r) {
        if (capacity[r] < 0) return of3dk::set_error("of3d: a quiver capacity must not be negative"), 0;
        if (capacity[r] > ((int64_t)1 << 56)) return of3dk::set_error("of3d: quiver capacity too large"), 0;
        words += 4 * (size_t)capacity[r];
    }
    return words;
}

// The lattices of the (checked) boxes as boxes of their own, (0, lz, 0, ly, 0, lx), planned as
// plan_boxes plans a reduction: workgroups per box, a workgroup's share below 2^31 points, the
// workspace words (one per wave).  dims NULL: the boxes against 2^31 alone.
int plan_lattices(const int64_t* rois, int n_roi, const int64_t* gap3, const int64_t* dims, int64_t* lat /* [n_roi][3] */,
                  int* nb, long long* woff, size_t* ws_words) {
    if (!gap3) return of3dk::set_error("of3d: null argument");
    if (of3dk::check_roi_count(rois, n_roi) != 0) return -1;
    for (int a = 0; a < 3; ++a)
        if (gap3[a] < 1) return of3dk::set_error("of3d: a quiver gap must be at least 1");
    int64_t lrois[kMaxRoi * 6];
    for (int r = 0; r < n_roi; ++r)
        for (int a = 0; a < 3; ++a) {
            const int64_t ext = of3dk::box_extent(rois, r, a, dims);
            if (ext < 0) return -1;
            lat[r * 3 + a] = (ext - 1) / gap3[a] + 1;
            lrois[r * 6 + 2 * a] = 0, lrois[r * 6 + 2 * a + 1] = lat[r * 3 + a];
        }
    return of3dk::plan_boxes(lrois, n_roi, nullptr, kSumWaves, nb, woff, ws_words);
}

}  // namespace

extern "C" {

size_t of3d_quiver_result_bytes(int n_roi, const int64_t* capacity) { return result_words(n_roi, capacity) * 8; }

size_t of3d_quiver_workspace_bytes(const int64_t* rois, int n_roi, const int64_t* gap3) {
    int64_t lat[kMaxRoi * 3];
    size_t words = 0;
    if (plan_lattices(rois, n_roi, gap3, nullptr, lat, nullptr, nullptr, &words) != 0) return 0;
    return words * 8;
}

int of3d_quiver_sample(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                       int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                       double tscale, const int64_t* rois, int n_roi, const int64_t* gap3, const int64_t* capacity,
                       const uint16_t* d_keep, void* d_result, void* workspace, void* stream) {
    if (!vx || !vy || !rois || !gap3 || !capacity || !d_result || !workspace || (!d_keep && (!rel || !d_thresh)))
        return of3dk::set_error("of3d: null argument");
    if (of3dk::check_volume(nz, ny, nx, !vz) != 0) return -1;
    if (vz && nz == 1) return of3dk::set_error("of3d: a 2D quiver sample (nz == 1) takes no vz");
    QvParams P{};
    P.sxy = xyscale, P.sz = zscale, P.st = tscale;
    const int64_t dims[3] = {nz, ny, nx};
    int64_t lat[kMaxRoi * 3];
    if (plan_lattices(rois, n_roi, gap3, dims, lat, P.nb, P.woff, nullptr) != 0) return -1;
    if (!result_words(n_roi, capacity)) return -1;
    const int max_nb = of3dk::fill_boxes(P, dims, rois, n_roi);
    for (int a = 0; a < 3; ++a) P.gap[a] = gap3[a] > INT32_MAX ? INT32_MAX : (int)gap3[a];
    long long off = kHead + (long long)n_roi * kRoiHead;
    for (int r = 0; r < n_roi; ++r) {
        for (int a = 0; a < 3; ++a) P.lat[r][a] = (int)lat[r * 3 + a];
        P.cap[r] = capacity[r], P.boff[r] = off;
        off += 4 * capacity[r];
    }
    hipStream_t s = (hipStream_t)stream;
    u64* ws = (u64*)workspace;
    u64* res = (u64*)d_result;
    const dim3 grid(max_nb, n_roi);
    of3dk::with_flow_types(v_f32, rel_f64, d_keep != nullptr, [&](auto vt, auto rt, auto masked_c) {
        using VT = decltype(vt);
        using RT = decltype(rt);
        constexpr bool M = decltype(masked_c)::value;
        hipLaunchKernelGGL((k_quiver_count<VT, RT, M>), grid, dim3(kSumThreads), 0, s, (const VT*)vx, (const VT*)vy,
                           (const VT*)vz, (const RT*)rel, (const RT*)d_thresh, d_keep, P, ws);
        hipLaunchKernelGGL(k_quiver_scan, dim3(n_roi), dim3(kScanThreads), 0, s, ws, P, d_thresh, rel_f64,
                           (long long)gap3[0], (long long)gap3[1], (long long)gap3[2], vz ? 1 : 0, res);
        hipLaunchKernelGGL((k_quiver_emit<VT, RT, M>), grid, dim3(kSumThreads), 0, s, (const VT*)vx, (const VT*)vy,
                           (const VT*)vz, (const RT*)rel, (const RT*)d_thresh, d_keep, P, (const u64*)ws, res);
    });
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

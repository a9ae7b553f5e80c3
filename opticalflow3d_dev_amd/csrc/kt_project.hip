// kt_project.hip — the projection maps (of3d_flow_project): per box of the frame summary and per
// axis one value per line of the box — the line's voxels in ascending order along the axis —
// for nine maps: the mask's footprint (the scripts' sum(relMask,3)), the valid count, the
// sequential sums of the masked physical velocities and of their magnitude, the maximum
// magnitude, and the maximum (max(myo,[],3)) and sum of an image volume of any input dtype.
// The sums are loops: s = 0.0, then s = s + v for k ascending, so a map does not depend on the
// launch shape.  Two line kernels serve the three axes:
//   k_project_lines (axes z, y)  one lane per line, the plane's pixels flattened in C order
//       over the lanes: consecutive lanes read consecutive x; a lane marches its line kVoxUnroll
//       voxels per trip, all loads before any arithmetic.
//   k_project_rows (axis x)      a workgroup takes kTileLines consecutive lines and walks them
//       kTileX voxels of x per step: the tile is loaded coalesced along x, each voxel's physical
//       values are formed by the lane that loaded it and parked in LDS (pitch kTileX + 1 words:
//       32 lanes reading one column touch 64 distinct banks), and lane (g, l) — group g of eight,
//       line l — adds column after column of one parked array to the one accumulator it owns.
//       The next tile's loads are in flight during the walk.
// A one-workgroup launch behind them writes the header and the maps' zero pads.  Every word of
// the result has exactly one writer; no atomics, no workspace.
// The mask source, the mask factor and the masking steps are summary_dev.hpp's, the box checks
// summary_host.hpp's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "summary_dev.hpp"

namespace {

using u64 = unsigned long long;

using of3dk::kMaxRoi, of3dk::kVoxUnroll;
constexpr int kHead = OF3D_PROJECT_HEAD_WORDS, kRoiHead = OF3D_PROJECT_ROI_WORDS;
constexpr int kMaps = 9;  // n_mask n_valid sum_vx sum_vy sum_vz sum_magnitude max_magnitude max_image sum_image
constexpr unsigned kMapBits = (1u << kMaps) - 1, kVzMap = 1u << 4, kImageMaps = 3u << 7;
constexpr int kLineThreads = 64;  // k_project_lines: one wave, so that a small plane still spreads over the CUs
constexpr int kPjThreads = 256;   // k_project_rows
constexpr int kTileLines = 32, kTileX = 32, kPitch = kTileX + 1;  // k_project_rows' tile
constexpr int kLoadRows = kPjThreads / kTileX;                    // tile rows loaded per pass of the workgroup
constexpr int kRowsPerLane = kTileLines / kLoadRows;
constexpr long long kMaxGrid = (1ll << 24) - 1;  // workgroups of a box and axis at most
constexpr u64 kNaNBits = 0x7FF8000000000000ull;

// np: the lines of the box along the axis = the elements of a map; nb (plan_boxes) 0: skipped
struct PjParams : of3dk::BoxParams {
    long long np[kMaxRoi][3];
    long long off[kMaxRoi][3];  // first result word of the first map of (box, axis); 0: none
    long long total;            // words of the result
    double sxy, sz, st;
    int axes, maps, has_vz, img_code;
};

// max(m, v) that ignores NaNs, from m = NaN: MATLAB's max, numpy's fmax
__device__ __forceinline__ double nan_max(double m, double v) { return (v > m || m != m) ? v : m; }

// element i of an image volume of dtype `code` (of3d_dtype) as a double; the frame ring keeps
// uint16 / uint32 frames in signed storage, the code says what the bits are
__device__ __forceinline__ double load_image(const void* __restrict__ img, int code, size_t i) {
    switch (code) {
        case OF3D_U8: return (double)((const uint8_t*)img)[i];
        case OF3D_U16: return (double)((const uint16_t*)img)[i];
        case OF3D_I16: return (double)((const int16_t*)img)[i];
        case OF3D_U32: return (double)((const uint32_t*)img)[i];
        case OF3D_I32: return (double)((const int32_t*)img)[i];
        case OF3D_F32: return (double)((const float*)img)[i];
        default: return ((const double*)img)[i];
    }
}

// Where the maps of one (box, axis) go: map k's element p
struct MapOut {
    u64* __restrict__ base;
    long long words;  // of a map, its pad included
    unsigned maps;

    __device__ __forceinline__ MapOut(u64* result, const PjParams& P, int roi, int axis)
        : base(result + P.off[roi][axis]), words((P.np[roi][axis] + 1) & ~1ll), maps((unsigned)P.maps) {}

    __device__ __forceinline__ void put(int k, long long p, u64 bits) const {
        if (maps >> k & 1) base[__popc(maps & ((1u << k) - 1)) * words + p] = bits;
    }
    __device__ __forceinline__ void put(int k, long long p, double v) const {
        put(k, p, (u64)__double_as_longlong(v));
    }
};

template <typename VT, typename RelT, bool Masked>
__device__ __forceinline__ of3dk::FlowFields<VT, RelT, Masked> flow_fields(const VT* vx, const VT* vy, const VT* vz,
                                                                           const RelT* rel, const RelT* thr_p,
                                                                           const uint16_t* keep, const PjParams& P,
                                                                           int roi) {
    return {vx,    vy,   vz,   rel, keep,         (Masked || !thr_p) ? 0.0 : (double)*thr_p,
            P.sxy, P.sz, P.st, roi, vz != nullptr};
}

// Axes z and y.  Grid (workgroups, box, axis 0 / 1); a lane owns pixel p of the plane — (y, x)
// for axis z, (z, x) for axis y — and marches its line.
template <typename VT, typename RelT, bool Masked, bool Img>
__global__ __launch_bounds__(kLineThreads) void k_project_lines(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                              const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                              const RelT* __restrict__ thr_p,
                                                              const uint16_t* __restrict__ keep,
                                                              const void* __restrict__ img, PjParams P,
                                                              u64* __restrict__ result) {
    const int roi = blockIdx.y, axis = blockIdx.z;
    if (!P.nb[roi] || !(P.axes >> axis & 1)) return;
    const long long p = (long long)blockIdx.x * kLineThreads + threadIdx.x;
    if (p >= P.np[roi][axis]) return;
    const auto F = flow_fields<VT, RelT, Masked>(vx, vy, vz, rel, thr_p, keep, P, roi);
    const int z0 = P.box[roi][0], y0 = P.box[roi][2], x0 = P.box[roi][4];
    const unsigned dx = P.box[roi][5] - x0;
    const size_t ny = P.ny, nx = P.nx;
    const size_t a = (size_t)(p / dx), x = (size_t)(p % dx);
    // the line's first voxel, the step to its next one and its length
    const size_t first = axis == 0 ? ((size_t)z0 * ny + y0 + a) * nx + x0 + x : ((z0 + a) * ny + y0) * nx + x0 + x;
    const size_t stride = axis == 0 ? ny * nx : nx;
    const unsigned len = axis == 0 ? P.box[roi][1] - z0 : P.box[roi][3] - y0;  // < 2^31: k + u cannot wrap
    long long n_mask = 0, n_valid = 0;
    double svx = 0.0, svy = 0.0, svz = 0.0, smag = 0.0, simg = 0.0;
    double mmag = __builtin_nan(""), mimg = __builtin_nan("");
    for (unsigned k = 0; k < len; k += kVoxUnroll) {
        of3dk::RawVoxel raw[kVoxUnroll];
        double im[kVoxUnroll];
#pragma unroll
        for (int u = 0; u < kVoxUnroll; ++u) {  // all loads before any arithmetic
            raw[u] = of3dk::RawVoxel{0.0, 0.0, 0.0, 0.0}, im[u] = 0.0;
            if (k + u < len) {
                const size_t i = first + (size_t)(k + u) * stride;
                raw[u] = of3dk::load_voxel(F, i);
                if constexpr (Img) im[u] = load_image(img, P.img_code, i);
            }
        }
#pragma unroll
        for (int u = 0; u < kVoxUnroll; ++u) {
            if (k + u >= len) continue;
            n_mask += of3dk::mask_factor(F, raw[u].r) != 0.0;
            const of3dk::Voxel v = of3dk::physical_voxel(F, raw[u]);
            if (v.sq == v.sq) {
                const double mag = sqrt(v.sq);
                n_valid += 1;
                svx = svx + v.vxp, svy = svy + v.vyp, svz = svz + v.vzp, smag = smag + mag;
                mmag = nan_max(mmag, mag);
            }
            if constexpr (Img) mimg = nan_max(mimg, im[u]), simg = simg + im[u];
        }
    }
    const MapOut out(result, P, roi, axis);
    out.put(0, p, (u64)n_mask), out.put(1, p, (u64)n_valid);
    out.put(2, p, svx), out.put(3, p, svy), out.put(4, p, svz), out.put(5, p, smag), out.put(6, p, mmag);
    if constexpr (Img) out.put(7, p, mimg), out.put(8, p, simg);
}

// Axis x.  Grid (workgroups, box); workgroup b takes lines [b * kTileLines, ...) of the box's
// dz * dy lines.  The parked arrays of a tile, one word per voxel: the three physical
// velocities (NaN bits in all three where the voxel is not valid), the magnitude — where the
// voxel is not valid the NaN bits with the mask bit in bit 0 — and the image value.  Thread t is
// loader of column t % 32 of rows t / 32 + 8 j, and owner (g, l) = (t / 32, t % 32):
//   g 0  n_mask, n_valid (of the magnitudes)   g 1 2 3  sum_vx, sum_vy, sum_vz
//   g 4  sum_magnitude   g 5  max_magnitude    g 6  max_image   g 7  sum_image
enum { kParkVx, kParkVy, kParkVz, kParkMag, kParkImg };
template <typename VT, typename RelT, bool Masked, bool Img>
__global__ __launch_bounds__(kPjThreads) void k_project_rows(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                             const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                             const RelT* __restrict__ thr_p,
                                                             const uint16_t* __restrict__ keep,
                                                             const void* __restrict__ img, PjParams P,
                                                             u64* __restrict__ result) {
    __shared__ u64 park[Img ? 5 : 4][kTileLines * kPitch];
    const int roi = blockIdx.y, axis = 2;
    const long long lines = P.np[roi][axis], line0 = (long long)blockIdx.x * kTileLines;
    if (!P.nb[roi] || line0 >= lines) return;  // the whole workgroup
    const int nl = lines - line0 < kTileLines ? (int)(lines - line0) : kTileLines;
    const auto F = flow_fields<VT, RelT, Masked>(vx, vy, vz, rel, thr_p, keep, P, roi);
    const int z0 = P.box[roi][0], y0 = P.box[roi][2], x0 = P.box[roi][4];
    const unsigned dy = P.box[roi][3] - y0, dx = P.box[roi][5] - x0;
    const size_t ny = P.ny, nx = P.nx;
    const int col = threadIdx.x % kTileX, row0 = threadIdx.x / kTileX;
    size_t base[kRowsPerLane];  // the first voxel of this loader's lines
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
        const long long line = line0 + row0 + j * kLoadRows;
        base[j] = line < lines ? ((size_t)(z0 + line / dy) * ny + (size_t)(y0 + line % dy)) * nx + x0 : 0;
    }
    of3dk::RawVoxel raw[kRowsPerLane];
    double im[kRowsPerLane];
    auto load_tile = [&](unsigned xt) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {
            raw[j] = of3dk::RawVoxel{0.0, 0.0, 0.0, 0.0}, im[j] = 0.0;
            if (row0 + j * kLoadRows < nl && xt + col < dx) {
                const size_t i = base[j] + xt + col;
                raw[j] = of3dk::load_voxel(F, i);
                if constexpr (Img) im[j] = load_image(img, P.img_code, i);
            }
        }
    };
    const int g = row0, l = col;
    const bool owner = l < nl && (Img || g < 6);
    const int src = g == 1 ? kParkVx : g == 2 ? kParkVy : g == 3 ? kParkVz : g < 6 ? kParkMag : kParkImg;
    const bool is_max = g == 5 || g == 6, add_all = g == 7;
    long long n_mask = 0, n_valid = 0;
    double s = is_max ? __builtin_nan("") : 0.0;
    load_tile(0);
    for (unsigned xt = 0; xt < dx; xt += kTileX) {
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j) {  // an element that was not loaded parks words nobody reads
            const double m = of3dk::mask_factor(F, raw[j].r);
            const of3dk::Voxel v = of3dk::physical_voxel(F, raw[j]);
            const bool valid = v.sq == v.sq;
            const int at = (row0 + j * kLoadRows) * kPitch + col;
            park[kParkVx][at] = valid ? (u64)__double_as_longlong(v.vxp) : kNaNBits;
            park[kParkVy][at] = valid ? (u64)__double_as_longlong(v.vyp) : kNaNBits;
            park[kParkVz][at] = valid ? (u64)__double_as_longlong(v.vzp) : kNaNBits;
            park[kParkMag][at] = valid ? (u64)__double_as_longlong(sqrt(v.sq)) : kNaNBits | (u64)(m != 0.0);
            if constexpr (Img) park[kParkImg][at] = (u64)__double_as_longlong(im[j]);
        }
        __syncthreads();
        if (xt + kTileX < dx) load_tile(xt + kTileX);  // in flight during the walk
        if (owner) {
            const u64* __restrict__ mine = &park[src][l * kPitch];
            const int cw = dx - xt < (unsigned)kTileX ? (int)(dx - xt) : kTileX;
#pragma unroll 8
            for (int c = 0; c < cw; ++c) {
                const u64 bits = mine[c];
                const double v = __longlong_as_double((long long)bits);
                const bool num = v == v;
                n_valid += num, n_mask += num | (bool)(bits & 1);
                s = is_max ? nan_max(s, v) : (add_all || num) ? s + v : s;
            }
        }
        __syncthreads();
    }
    if (!owner) return;
    const MapOut out(result, P, roi, axis);
    const long long p = line0 + l;
    if (g == 0)
        out.put(0, p, (u64)n_mask), out.put(1, p, (u64)n_valid);
    else
        out.put(g + 1, p, s);
}

// The header and the maps' zero pads, by one workgroup behind the line kernels on the same stream
__global__ void k_project_head(PjParams P, const void* thr_p, int rel_f64, u64* __restrict__ result) {
    const int t = threadIdx.x;
    if (t < P.n_roi) {
        u64* h = result + kHead + (size_t)t * kRoiHead;
        for (int a = 0; a < 3; ++a) h[2 * a] = (u64)P.np[t][a], h[2 * a + 1] = (u64)P.off[t][a];
    }
    for (int i = t; i < P.n_roi * 3 * kMaps; i += blockDim.x) {
        const int r = i / (3 * kMaps), a = i / kMaps % 3, k = i % kMaps;
        if (P.off[r][a] && (P.np[r][a] & 1) && (P.maps >> k & 1)) MapOut(result, P, r, a).put(k, P.np[r][a], (u64)0);
    }
    if (t == 0) {
        double thr = __builtin_nan("");
        if (thr_p) thr = rel_f64 ? *(const double*)thr_p : (double)*(const float*)thr_p;
        result[0] = (u64)__double_as_longlong(thr);
        result[1] = (u64)P.n_roi, result[2] = (u64)P.axes, result[3] = (u64)(unsigned)P.maps;
        result[4] = (u64)P.has_vz, result[5] = (u64)((P.maps & kImageMaps) ? P.img_code : 0);
        result[6] = (u64)P.total, result[7] = 0;
    }
}

// The request checked, the boxes checked (dims NULL: against 2^31 alone) and the result laid
// out: P's nb (0 for a skipped box), np, off, total; wg[a]: the workgroups of axis a's launch
// (the most any box needs; 0: the axis is not asked for).  -1 with the error set.
int plan_project(const int64_t* rois, int n_roi, const int64_t* dims, int axes, int maps, int has_vz, int img_code,
                 PjParams& P, long long (&wg)[3]) {
    if (of3dk::plan_boxes(rois, n_roi, dims, 0, P.nb) != 0) return -1;
    const unsigned m = (unsigned)maps, skip = m >> OF3D_PROJECT_SKIP_SHIFT;
    if (!(m & kMapBits) || (m & 0xFFFFu & ~kMapBits) || skip >> n_roi)
        return of3dk::set_error("of3d: project maps: bits 0..8, one at least, and the boxes' skip bits");
    if (skip == (1u << n_roi) - 1) return of3dk::set_error("of3d: every box of the projection is skipped");
    if (axes < 1 || axes > 7) return of3dk::set_error("of3d: project axes: bits 0..2 (z y x), one at least");
    if (!has_vz && (axes & 1)) return of3dk::set_error("of3d: a 2D projection has no z axis");
    if (!has_vz && (m & kVzMap)) return of3dk::set_error("of3d: a 2D projection has no sum_vz");
    if (img_code < 0 || img_code > OF3D_F64) return of3dk::set_error("of3d: project image dtype: an of3d_dtype or 0");
    if ((m & kImageMaps) && !img_code) return of3dk::set_error("of3d: the image maps of a projection need an image");
    const long long n_maps = __builtin_popcount(m & kMapBits);
    long long off = kHead + (long long)n_roi * kRoiHead;
    wg[0] = wg[1] = wg[2] = 0;
    for (int r = 0; r < n_roi; ++r) {
        long long ext[3];
        for (int a = 0; a < 3; ++a) ext[a] = rois[r * 6 + 2 * a + 1] - rois[r * 6 + 2 * a];
        if (skip >> r & 1) P.nb[r] = 0;
        for (int a = 0; a < 3; ++a) {
            P.np[r][a] = ext[(a + 1) % 3] * ext[(a + 2) % 3];
            P.off[r][a] = 0;
            if (!P.nb[r] || !(axes >> a & 1)) continue;
            const int per = a == 2 ? kTileLines : kLineThreads;
            const long long n = (P.np[r][a] + per - 1) / per;
            if (n > kMaxGrid) return of3dk::set_error("of3d: ROI too large (lines of a projection)");
            wg[a] = n > wg[a] ? n : wg[a];
            P.off[r][a] = off;
            off += n_maps * ((P.np[r][a] + 1) & ~1ll);
        }
    }
    P.total = off;
    P.axes = axes, P.maps = maps, P.has_vz = has_vz ? 1 : 0, P.img_code = img_code;
    return 0;
}

}  // namespace

extern "C" {

size_t of3d_flow_project_result_bytes(const int64_t* rois, int n_roi, int axes, int maps, int has_vz,
                                      int image_dtype) {
    PjParams P{};
    long long wg[3];
    if (plan_project(rois, n_roi, nullptr, axes, maps, has_vz, image_dtype, P, wg) != 0) return 0;
    return (size_t)P.total * 8;
}

int of3d_flow_project(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                      int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                      double tscale, const int64_t* rois, int n_roi, int axes, int maps, const void* d_image,
                      int image_dtype, const uint16_t* d_keep, void* d_result, void* stream) {
    if (!vx || !vy || !rois || !d_result || (!d_keep && (!rel || !d_thresh)))
        return of3dk::set_error("of3d: null argument");
    if (of3dk::check_volume(nz, ny, nx, !vz) != 0) return -1;
    if (vz && nz == 1) return of3dk::set_error("of3d: a 2D projection (nz == 1) takes no vz");
    if ((uintptr_t)d_result % 16) return of3dk::set_error("of3d: the projection result must be 16-byte aligned");
    PjParams P{};
    long long wg[3];
    const int64_t dims[3] = {nz, ny, nx};
    if (plan_project(rois, n_roi, dims, axes, maps, vz != nullptr, d_image ? image_dtype : 0, P, wg) != 0) return -1;
    of3dk::fill_boxes(P, dims, rois, n_roi);
    P.sxy = xyscale, P.sz = zscale, P.st = tscale;
    hipStream_t s = (hipStream_t)stream;
    u64* res = (u64*)d_result;
    const bool image = (unsigned)maps & kImageMaps;
    const long long wg_zy = wg[0] > wg[1] ? wg[0] : wg[1];
    of3dk::with_flow_types(v_f32, rel_f64, d_keep != nullptr, [&](auto vt, auto rt, auto masked_c) {
        using VT = decltype(vt);
        using RT = decltype(rt);
        constexpr bool M = decltype(masked_c)::value;
        auto launch = [&](auto img_c) {
            constexpr bool I = decltype(img_c)::value;
            if (wg_zy)
                hipLaunchKernelGGL((k_project_lines<VT, RT, M, I>), dim3((unsigned)wg_zy, n_roi, 2), dim3(kLineThreads), 0,
                                   s, (const VT*)vx, (const VT*)vy, (const VT*)vz, (const RT*)rel,
                                   (const RT*)d_thresh, d_keep, d_image, P, res);
            if (wg[2])
                hipLaunchKernelGGL((k_project_rows<VT, RT, M, I>), dim3((unsigned)wg[2], n_roi), dim3(kPjThreads), 0, s,
                                   (const VT*)vx, (const VT*)vy, (const VT*)vz, (const RT*)rel, (const RT*)d_thresh,
                                   d_keep, d_image, P, res);
        };
        if (image)
            launch(std::true_type{});
        else
            launch(std::false_type{});
    });
    hipLaunchKernelGGL(k_project_head, dim3(1), dim3(64), 0, s, P, d_thresh, rel_f64, res);
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

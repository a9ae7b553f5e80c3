// kt_export.hip — the field export (of3d_field_export): the fields cropped to the boxes of the
// frame summary, masked as the reference's scripts mask them right after loading them
// (vx.*relMask./relMask*xyscale/tscale in plot_figure3 / 4 / 5, vx.*relMask in
// plot_FigureS2_dt.m:123, the notebooks' vx*relMask; vx[vx==0]=nan), in physical units,
// optionally narrowed to float32, as compact blocks behind a small header.  A pure map in one
// launch, grid (workgroups, box, field): a block is cut into 16-byte groups of output (2 fp64 or
// 4 fp32 consecutive elements), workgroup b of a box's nb takes groups [b*ng/nb, (b+1)*ng/nb), a
// lane one group per step — one aligned 16-byte store whatever x0 and dx are; the group may
// straddle a row end of the box, so the source address is formed per element.  The last group of
// a block carries its zero pad; a one-workgroup launch behind it on the same stream writes the
// header.  Every byte of the result has exactly one writer.
// The mask source, the mask factor and the masking steps are summary_dev.hpp's, the checks and
// the workgroup plan summary_host.hpp's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "summary_dev.hpp"

namespace {

using u64 = unsigned long long;

using of3dk::kSumThreads, of3dk::kMaxRoi;  // summary_host.hpp
constexpr int kHead = OF3D_EXPORT_HEAD_WORDS, kRoiHead = OF3D_EXPORT_ROI_WORDS;
constexpr int kFields = 4;  // vx vy vz rel
constexpr unsigned kFieldBits = (1u << kFields) - 1;

// nb: the workgroups of a box (plan_boxes; 0: the box is skipped).
struct ExParams : of3dk::BoxParams {
    long long n[kMaxRoi];             // voxels of the box
    long long off[kMaxRoi][kFields];  // first result word of the box's block of a field; 0: none
    long long total;                  // words of the result
    double sxy, sz, st;
    int fields, mask_mode, physical, out_f32, has_vz;
    int esz_v, esz_r;  // bytes of an element of the velocity blocks / of the rel block
};

template <int Bytes>
using bits_t = std::conditional_t<Bytes == 4, uint32_t, u64>;

template <typename T>
__device__ __forceinline__ T from_bits(bits_t<sizeof(T)> b) {
    return __builtin_bit_cast(T, b);
}

// One field of box `roi`: this workgroup's groups of the block at dst.  Vel: a velocity component
// (masked by mask_mode, scaled by `scale` when physical) — else rel, the plain crop.
template <typename InT, typename OutT, bool Vel, typename VT, typename RelT, bool Masked>
__device__ __forceinline__ void export_block(const InT* __restrict__ src, OutT* __restrict__ dst,
                                             const of3dk::FlowFields<VT, RelT, Masked>& F, const ExParams& P, int roi,
                                             double scale) {
    using IB = bits_t<sizeof(InT)>;
    using OB = bits_t<sizeof(OutT)>;
    constexpr int G = 16 / (int)sizeof(OutT);
    struct alignas(16) Group {
        OB v[G];
    };
    const int nb = P.nb[roi], mode = Vel ? P.mask_mode : 0;
    const bool physical = Vel && P.physical;
    const bool copy = sizeof(InT) == sizeof(OutT) && mode == 0 && !physical;  // no arithmetic: the bits
    const long long n = P.n[roi], ng = (n + G - 1) / G;
    const long long g0 = ng * blockIdx.x / nb, g1 = ng * (blockIdx.x + 1) / nb;
    const int z0 = P.box[roi][0], y0 = P.box[roi][2], x0 = P.box[roi][4];
    const unsigned dy = P.box[roi][3] - y0, dx = P.box[roi][5] - x0;
    const size_t ny = P.ny, nx = P.nx;
    // the first element of this lane's first group, then kSumThreads groups per step
    const long long e0 = g0 * G;
    of3dk::BoxWalk w(dy, dx, e0 / dx, (unsigned)(e0 % dx) + threadIdx.x * G, kSumThreads * G);
    const IB* __restrict__ sb = reinterpret_cast<const IB*>(src);
    Group* __restrict__ db = reinterpret_cast<Group*>(dst);
    for (long long g = g0 + threadIdx.x; g < g1; g += kSumThreads) {
        IB raw[G];
        double r[G];
        unsigned x = w.x, y = w.y, z = w.z;
#pragma unroll
        for (int k = 0; k < G; ++k) {  // all loads before any arithmetic
            raw[k] = 0, r[k] = 0.0;
            if (g * G + k < n) {
                const size_t i = ((size_t)(z0 + z) * ny + (y0 + y)) * nx + (x0 + x);
                raw[k] = sb[i];
                if (mode != 0) r[k] = of3dk::load_mask(F, i);
            }
            if (++x == dx) {
                x = 0;
                if (++y == dy) y = 0, ++z;
            }
        }
        w.advance();
        Group out;
#pragma unroll
        for (int k = 0; k < G; ++k) {
            if (g * G + k >= n) {
                out.v[k] = 0;  // the pad
            } else if (copy) {
                out.v[k] = (OB)raw[k];
            } else {
                double v = (double)from_bits<InT>(raw[k]);
                const double m = of3dk::mask_factor(F, r[k]);
                if (mode == 1)
                    v = (v * m) / m;
                else if (mode == 2)
                    v = v * m;
                else if (mode == 3)
                    v = of3dk::zeroed_to_nan(v, m);
                if (physical) v = of3dk::physical_units(v, scale, F.st);
                out.v[k] = __builtin_bit_cast(OB, (OutT)v);
            }
        }
        db[g] = out;
    }
}

// Grid (max workgroups of a box, n_roi, kFields).  Masked: the mask factor of a voxel is bit `roi`
// of keep (of3d_mask_open) instead of rel > thr.  Narrow: float32 blocks whatever the fields are.
template <typename VT, typename RelT, bool Masked, bool Narrow>
__global__ __launch_bounds__(kSumThreads) void k_field_export(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                              const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                              const RelT* __restrict__ thr_p,
                                                              const uint16_t* __restrict__ keep, ExParams P,
                                                              u64* __restrict__ result) {
    const int roi = blockIdx.y, f = blockIdx.z;
    if ((int)blockIdx.x >= P.nb[roi] || !(P.fields >> f & 1)) return;
    using VO = std::conditional_t<Narrow, float, VT>;
    using RO = std::conditional_t<Narrow, float, RelT>;
    const of3dk::FlowFields<VT, RelT, Masked> F{
        vx,    vy,   vz,   rel, keep,         (Masked || !thr_p) ? 0.0 : (double)*thr_p,
        P.sxy, P.sz, P.st, roi, vz != nullptr};
    u64* dst = result + P.off[roi][f];
    switch (f) {
        case 0: export_block<VT, VO, true>(vx, (VO*)dst, F, P, roi, P.sxy); break;
        case 1: export_block<VT, VO, true>(vy, (VO*)dst, F, P, roi, P.sxy); break;
        case 2: export_block<VT, VO, true>(vz, (VO*)dst, F, P, roi, P.sz); break;
        default: export_block<RelT, RO, false>(rel, (RO*)dst, F, P, roi, 1.0); break;
    }
}

// The header, by one workgroup behind k_field_export on the same stream: the boxes' words (a
// skipped box: its voxel count and no offsets) and the head.
__global__ void k_export_head(ExParams P, const void* thr_p, int rel_f64, u64* __restrict__ result) {
    const int t = threadIdx.x;
    if (t < P.n_roi) {
        u64* h = result + kHead + (size_t)t * kRoiHead;
        h[0] = (u64)P.n[t], h[1] = (u64)(P.esz_v + 256 * P.esz_r);
        for (int k = 0; k < kFields; ++k) h[2 + k] = (u64)P.off[t][k];
    }
    if (t == 0) {
        double thr = __builtin_nan("");
        if (thr_p) thr = rel_f64 ? *(const double*)thr_p : (double)*(const float*)thr_p;
        result[0] = (u64)__double_as_longlong(thr);
        result[1] = (u64)P.n_roi, result[2] = (u64)(unsigned)P.fields, result[3] = (u64)P.mask_mode;
        result[4] = (u64)P.physical, result[5] = (u64)P.out_f32, result[6] = (u64)P.has_vz;
        result[7] = (u64)P.total;
    }
}

// The boxes checked (dims NULL: against 2^31 alone) and the result laid out: P's nb (0 for a
// skipped box), n, off, total, esz_*.  -1 with the error set.
int plan_export(const int64_t* rois, int n_roi, const int64_t* dims, int fields, int v_f32, int rel_f64, int out_f32,
                ExParams& P) {
    if (of3dk::plan_boxes(rois, n_roi, dims, 0, P.nb) != 0) return -1;
    const unsigned f = (unsigned)fields, skip = f >> OF3D_EXPORT_SKIP_SHIFT;
    if (!(f & kFieldBits) || (f & 0xFFFFu & ~kFieldBits) || skip >> n_roi)
        return of3dk::set_error("of3d: export fields: bits 0..3 (vx vy vz rel), one at least, and the boxes' skip bits");
    if (skip == (1u << n_roi) - 1) return of3dk::set_error("of3d: every box of the export is skipped");
    P.esz_v = (out_f32 || v_f32) ? 4 : 8, P.esz_r = (out_f32 || !rel_f64) ? 4 : 8;
    long long off = kHead + (long long)n_roi * kRoiHead;
    for (int r = 0; r < n_roi; ++r) {
        P.n[r] = 1;
        for (int a = 0; a < 3; ++a) P.n[r] *= rois[r * 6 + 2 * a + 1] - rois[r * 6 + 2 * a];
        if (skip >> r & 1) P.nb[r] = 0;
        for (int k = 0; k < kFields; ++k) {
            P.off[r][k] = 0;
            if (!P.nb[r] || !(f >> k & 1)) continue;
            P.off[r][k] = off;
            off += 2 * ((P.n[r] * (k == 3 ? P.esz_r : P.esz_v) + 15) / 16);
        }
    }
    P.total = off;
    return 0;
}

}  // namespace

extern "C" {

size_t of3d_field_export_result_bytes(const int64_t* rois, int n_roi, int fields, int v_f32, int rel_f64, int out_f32) {
    ExParams P{};
    if (plan_export(rois, n_roi, nullptr, fields, v_f32, rel_f64, out_f32, P) != 0) return 0;
    return (size_t)P.total * 8;
}

int of3d_field_export(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                      int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                      double tscale, const int64_t* rois, int n_roi, int fields, int mask_mode, int physical, int out_f32,
                      const uint16_t* d_keep, void* d_result, void* stream) {
    if (mask_mode < 0 || mask_mode > 3) return of3dk::set_error("of3d: export mask_mode must be 0, 1, 2 or 3");
    const bool vel = fields & 7;
    if (!rois || !d_result || ((fields & 1) && !vx) || ((fields & 2) && !vy) || ((fields & 8) && !rel) ||
        (vel && mask_mode && !d_keep && (!rel || !d_thresh)))
        return of3dk::set_error("of3d: null argument");
    if (of3dk::check_volume(nz, ny, nx, !vz) != 0) return -1;
    if (vz && nz == 1) return of3dk::set_error("of3d: a 2D field export (nz == 1) takes no vz");
    if ((fields & 4) && !vz) return of3dk::set_error("of3d: a 2D field export (d_vz NULL) has no vz to export");
    if ((uintptr_t)d_result % 16) return of3dk::set_error("of3d: the export result must be 16-byte aligned");
    ExParams P{};
    const int64_t dims[3] = {nz, ny, nx};
    if (plan_export(rois, n_roi, dims, fields, v_f32, rel_f64, out_f32, P) != 0) return -1;
    const int max_nb = of3dk::fill_boxes(P, dims, rois, n_roi);
    P.sxy = xyscale, P.sz = zscale, P.st = tscale;
    P.fields = fields, P.mask_mode = mask_mode, P.physical = physical ? 1 : 0, P.out_f32 = out_f32 ? 1 : 0;
    P.has_vz = vz ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    u64* res = (u64*)d_result;
    const dim3 grid(max_nb, n_roi, kFields);
    // the mask source matters to the velocity blocks of a masked mode alone
    const bool masked = d_keep != nullptr && vel && mask_mode;
    of3dk::with_flow_types(v_f32, rel_f64, masked, [&](auto vt, auto rt, auto masked_c) {
        using VT = decltype(vt);
        using RT = decltype(rt);
        constexpr bool M = decltype(masked_c)::value;
        if (out_f32)
            hipLaunchKernelGGL((k_field_export<VT, RT, M, true>), grid, dim3(kSumThreads), 0, s, (const VT*)vx,
                               (const VT*)vy, (const VT*)vz, (const RT*)rel, (const RT*)d_thresh, d_keep, P, res);
        else
            hipLaunchKernelGGL((k_field_export<VT, RT, M, false>), grid, dim3(kSumThreads), 0, s, (const VT*)vx,
                               (const VT*)vy, (const VT*)vz, (const RT*)rel, (const RT*)d_thresh, d_keep, P, res);
    });
    hipLaunchKernelGGL(k_export_head, dim3(1), dim3(64), 0, s, P, d_thresh, rel_f64, res);
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

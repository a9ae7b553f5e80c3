#pragma once
// summary_dev.hpp — the per-voxel device helpers shared by the frame summary (kt_summary.hip:
// k_sum_boxes), the projected flow (kt_axes.hip: k_proj_boxes), the magnitude-weighted
// histograms (kt_whist.hip: k_whist_boxes), the two-channel comparison (kt_pair.hip:
// k_pair_boxes), the quiver samples (kt_quiver.hip: walk_wave), the contractility
// (kt_contract.hip: k_ct_boxes), the spread (kt_spread.hip: k_spread_boxes), the reliability
// profile (kt_relsel.hip: k_rp_boxes) and the field export (kt_export.hip: export_block): one statement of the masking arithmetic, the histogram bin
// search, the walk over a box, a workgroup's share of a box, the loop over its voxels and the
// reduction of its sums, so the passes cannot drift apart.  The host side (volume and box
// checks, workgroup plan, histogram plan, edge upload, type dispatch) is summary_host.hpp's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "summary_host.hpp"

namespace of3dk {

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

// example_analysis_script.ipynb cell 5 for one component, step by step (kt_export.hip applies the
// steps one at a time): v * mask (numpy: v * bool mask) with exact zeros -> NaN, and the
// physical units (v * scale) / tscale
__device__ __forceinline__ double zeroed_to_nan(double v, double m) {
    v = v * m;
    if (v == 0.0) v = __builtin_nan("");
    return v;
}

__device__ __forceinline__ double physical_units(double v, double scale, double tscale) {
    return (v * scale) / tscale;
}

__device__ __forceinline__ double masked_velocity(double v, double m, double scale, double tscale) {
    return physical_units(zeroed_to_nan(v, m), scale, tscale);
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

// Workgroup blockIdx.x's share of box `roi` (rows [b*R/nb, (b+1)*R/nb) of its R = dz*dy rows) and
// this thread's walk over it, kSumThreads voxels per step.
struct BoxShare {
    int z0, y0, x0, ny, nx;
    unsigned dy, dx;
    long long count;  // this workgroup's voxels (< 2^31: checked on the host)
    BoxWalk w;        // this thread's voxel as (z, y, x) inside the box

    // the walk's voxel in the whole volume
    __device__ __forceinline__ size_t index() const { return ((size_t)(z0 + w.z) * ny + (y0 + w.y)) * nx + (x0 + w.x); }
};

__device__ __forceinline__ BoxShare box_share(const BoxParams& P, int roi, int nb) {
    const int z0 = P.box[roi][0], y0 = P.box[roi][2], x0 = P.box[roi][4];
    const unsigned dy = P.box[roi][3] - y0, dx = P.box[roi][5] - x0;
    const long long R = (long long)(P.box[roi][1] - z0) * dy;
    const long long r0 = R * blockIdx.x / nb, r1 = R * (blockIdx.x + 1) / nb;
    return {z0, y0, x0, P.ny, P.nx, dy, dx, (r1 - r0) * dx, BoxWalk(dy, dx, r0, threadIdx.x, kSumThreads)};
}

// ---------------------------------------------------------------------------
// The voxels of a flow pass: what the pass takes of the fields, one voxel's load and masking
// arithmetic, and the two loops over a workgroup's share of a box.
// ---------------------------------------------------------------------------
// Masked: the mask factor of a voxel is bit `roi` of keep (of3d_mask_open, of3d_mask_largest)
// instead of rel > thr.  is3: the pass has a vz.
template <typename VT, typename RelT, bool Masked>
struct FlowFields {
    const VT *__restrict__ vx, *__restrict__ vy, *__restrict__ vz;
    const RelT* __restrict__ rel;
    const uint16_t* __restrict__ keep;
    double thr, sxy, sz, st;
    int roi;
    bool is3;
};

struct RawVoxel {
    double x, y, z, r;  // the loaded velocity; r: the mask bit as 0 / 1 (Masked) or rel
};

struct Voxel {
    double vxp, vyp, vzp;  // physical velocity, NaN outside the mask and where it was an exact zero
    double xy2, sq;        // vxp^2 + vyp^2; the magnitude's square: xy2 (+ vzp^2 with a vz)
};

// RawVoxel's r of voxel i, and the mask factor (0.0 / 1.0) it stands for
template <typename VT, typename RelT, bool Masked>
__device__ __forceinline__ double load_mask(const FlowFields<VT, RelT, Masked>& F, size_t i) {
    if constexpr (Masked)
        return (F.keep[i] >> F.roi & 1) ? 1.0 : 0.0;
    else
        return (double)F.rel[i];
}

template <typename VT, typename RelT, bool Masked>
__device__ __forceinline__ double mask_factor(const FlowFields<VT, RelT, Masked>& F, double r) {
    return Masked ? r : (r > F.thr) ? 1.0 : 0.0;  // numpy: v * bool mask
}

template <typename VT, typename RelT, bool Masked>
__device__ __forceinline__ RawVoxel load_voxel(const FlowFields<VT, RelT, Masked>& F, size_t i) {
    RawVoxel v{0.0, 0.0, 0.0, 0.0};
    v.r = load_mask(F, i);
    v.x = (double)F.vx[i];
    v.y = (double)F.vy[i];
    if (F.is3) v.z = (double)F.vz[i];
    return v;
}

// The voxel is valid <=> its magnitude is not NaN (badRows = isnan(mag)) <=> sq == sq: a sum of
// squares is NaN or >= 0, so its root is NaN exactly where it is.  The magnitude is sqrt(sq).
template <typename VT, typename RelT, bool Masked>
__device__ __forceinline__ Voxel physical_voxel(const FlowFields<VT, RelT, Masked>& F, const RawVoxel& raw) {
    const double m = mask_factor(F, raw.r);
    Voxel v;
    v.vxp = masked_velocity(raw.x, m, F.sxy, F.st);
    v.vyp = masked_velocity(raw.y, m, F.sxy, F.st);
    v.vzp = F.is3 ? masked_velocity(raw.z, m, F.sz, F.st) : 0.0;
    v.xy2 = v.vxp * v.vxp + v.vyp * v.vyp;
    v.sq = F.is3 ? v.xy2 + v.vzp * v.vzp : v.xy2;
    return v;
}

// One trip of a thread over its share: kVoxUnroll voxels kSumThreads apart, the first of them
// element e of the share, all loads issued before any arithmetic.  An element past the end is
// not loaded: in[u] false and zeros, which are never valid (a zero velocity becomes NaN).
// k[u]: the voxel inside the box (x y z).
constexpr int kVoxUnroll = 4;
template <typename VT, typename RelT, bool Masked>
__device__ __forceinline__ void load_trip(const FlowFields<VT, RelT, Masked>& F, BoxShare& sh, long long e,
                                          RawVoxel (&raw)[kVoxUnroll], bool (&in)[kVoxUnroll],
                                          unsigned (&k)[kVoxUnroll][3]) {
#pragma unroll
    for (int u = 0; u < kVoxUnroll; ++u) {
        in[u] = e + (long long)u * kSumThreads < sh.count;
        raw[u] = RawVoxel{0.0, 0.0, 0.0, 0.0};
        k[u][0] = sh.w.x, k[u][1] = sh.w.y, k[u][2] = sh.w.z;
        if (in[u]) raw[u] = load_voxel(F, sh.index());
        sh.w.advance();
    }
}

// body(voxel, x, y, z) for every valid voxel of the share, x y z inside the box; a thread takes
// its voxels in ascending order and leaves once it has none left.
template <typename VT, typename RelT, bool Masked, typename Body>
__device__ __forceinline__ void for_valid_voxels(const FlowFields<VT, RelT, Masked>& F, BoxShare& sh, Body&& body) {
    for (long long e = threadIdx.x; e < sh.count; e += (long long)kVoxUnroll * kSumThreads) {
        RawVoxel raw[kVoxUnroll];
        bool in[kVoxUnroll];
        unsigned k[kVoxUnroll][3];
        load_trip(F, sh, e, raw, in, k);
#pragma unroll
        for (int u = 0; u < kVoxUnroll; ++u) {
            if (!in[u]) continue;
            const Voxel v = physical_voxel(F, raw[u]);
            if (v.sq == v.sq) body(v, k[u][0], k[u][1], k[u][2]);
        }
    }
}

// The wave-uniform form, for bodies with ballots and shuffles: the same trips in every lane and
// body(voxel, valid) for every element, those past the end included (not valid).
template <typename VT, typename RelT, bool Masked, typename Body>
__device__ __forceinline__ void for_voxels_uniform(const FlowFields<VT, RelT, Masked>& F, BoxShare& sh, Body&& body) {
    for (long long e0 = 0; e0 < sh.count; e0 += (long long)kVoxUnroll * kSumThreads) {
        RawVoxel raw[kVoxUnroll];
        bool in[kVoxUnroll];
        unsigned k[kVoxUnroll][3];
        load_trip(F, sh, e0 + threadIdx.x, raw, in, k);
#pragma unroll
        for (int u = 0; u < kVoxUnroll; ++u) {
            const Voxel v = physical_voxel(F, raw[u]);
            body(v, v.sq == v.sq);
        }
    }
}

// The fixed shuffle tree over a wave's 64 lanes, all of them active: lane 0 returns the sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// A workgroup's N sums into its workspace slot, called by all kSumThreads threads (full EXEC):
// per sum wave_sum's tree over the lanes, then the waves' partials added in wave order.
template <int N>
__device__ __forceinline__ void reduce_to_slot(const double (&acc)[N], double (*wsum)[N], double* __restrict__ slot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const double v = wave_sum(acc[q]);
        if (lane == 0) wsum[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double v = wsum[0][threadIdx.x];
        for (int j = 1; j < kSumWaves; ++j) v += wsum[j][threadIdx.x];
        slot[threadIdx.x] = v;
    }
}

// A workgroup's LDS histogram (counts) into a box's result words by 64-bit integer atomics
__device__ __forceinline__ void flush_hist(const unsigned* hist, int ntot, unsigned long long* __restrict__ dst) {
    for (int i = threadIdx.x; i < ntot; i += kSumThreads)
        if (hist[i]) atomicAdd(&dst[i], (unsigned long long)hist[i]);
}

// The final pass of a box, one workgroup of kFinalThreads: G sums of each of its nb slots (slot
// b's at src + b * Stride) staged in LDS (s: nb * G doubles), each then added in slot order by
// one thread and stored as its bits in dst[0 .. G).
constexpr int kFinalThreads = 256;
template <int G, int Stride>
__device__ __forceinline__ void add_slots(const double* __restrict__ src, int nb, double* s,
                                          unsigned long long* __restrict__ dst) {
    for (int i = threadIdx.x; i < nb * G; i += kFinalThreads) s[i] = src[(size_t)(i / G) * Stride + i % G];
    __syncthreads();
    if (threadIdx.x < G) {
        double v = s[threadIdx.x];
        for (int b = 1; b < nb; ++b) v += s[b * G + threadIdx.x];
        dst[threadIdx.x] = (unsigned long long)__double_as_longlong(v);
    }
}

}  // namespace of3dk

#pragma once
// of3d_general.hpp — the general-radius path, the pointwise 2D solve, of3d_rel3d's kernel and the
// downstream statistics (pipeline overview: of3d_common.hpp).
#include <type_traits>

#include "of3d_common.hpp"
#include "of3d_solve.hpp"

namespace {

// ---------------------------------------------------------------------------
// General-radius path (any xyzSig / wSig the reference accepts, calc_flow.py:230-267,
// beyond the tiled kernels' LDS limits): every 1-D pass as its own streaming kernel
// straight from global memory (L2), one output per thread, the same scipy order and
// global-edge clamping; products and solves pointwise.  Not tuned: it exists so that no
// parameter the reference takes is refused.
// ---------------------------------------------------------------------------
template <typename T, typename F>
__global__ __launch_bounds__(256) void k_cast_gen(const T* __restrict__ in, F* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (F)in[i];
}

// out[q] (planes [q0, q1), origin out_z0) = pass along `axis` (0 x, 1 y, 2 z) of in (origin
// in_z0); z indices clamp to [0, zhi); half taps h[0..r] (h[k] = w[r - k]); anti: lo - hi
template <typename F>
__global__ __launch_bounds__(256) void k_corr_gen(const F* __restrict__ in, int in_z0, F* __restrict__ out, int out_z0,
                                                  int q0, int q1, int ny, int nx, int axis, const F* __restrict__ h,
                                                  int r, int anti, int zhi) {
    const size_t plane = (size_t)ny * nx, n = (size_t)(q1 - q0) * plane;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int q = q0 + (int)(i / plane);
        const size_t rem = i % plane;
        const int y = (int)(rem / nx), x = (int)(rem % nx);
        auto at = [&](int d) -> F {
            int zz = q, yy = y, xx = x;
            if (axis == 0)
                xx = clampi(x + d, 0, nx - 1);
            else if (axis == 1)
                yy = clampi(y + d, 0, ny - 1);
            else
                zz = clampi(q + d, 0, zhi - 1);
            return in[(size_t)(zz - in_z0) * plane + (size_t)yy * nx + xx];
        };
        F o = at(0) * h[0];
        for (int k = r; k >= 1; --k) o = o + (anti ? (at(-k) - at(k)) : (at(-k) + at(k))) * h[k];
        out[(size_t)(q - out_z0) * plane + rem] = o;
    }
}

// the structure-tensor products (tables as k_prod_wyx): P[p] = G[a(p)] * G[b(p)], n points
template <typename F>
__global__ __launch_bounds__(256) void k_prod_gen(const F* __restrict__ G, F* __restrict__ P, size_t fs, size_t n,
                                                  int np) {
    const unsigned long long pa = np == 9 ? 0x311222312ull : 0x12212ull, pb = np == 9 ? 0x313231000ull : 0x12100ull;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        for (int p = 0; p < np; ++p)
            P[p * fs + i] = G[((pa >> (4 * p)) & 15u) * fs + i] * G[((pb >> (4 * p)) & 15u) * fs + i];
}

// Reliability of given structure tensors (of3d_rel3d): field-major [6][n] in the order
// x2 y2 z2 xy xz yz, the same eigmin3 instance the solve kernels use for RelT
template <typename RelT>
__global__ __launch_bounds__(256) void k_rel3d(const double* __restrict__ T, size_t n, RelT* __restrict__ rel) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        rel[i] = (RelT)eigmin3<std::is_same_v<RelT, double>>(T[i], T[n + i], T[2 * n + i], T[3 * n + i],
                                                             T[4 * n + i], T[5 * n + i]);
}

// 3D solve + reliability from the nine windowed fields (order tx ty tz xy xz x2 yz y2 z2)
template <typename F, typename RelT>
__global__ __launch_bounds__(256) void k_solve3_gen(const F* __restrict__ W, size_t fs, size_t n, F* __restrict__ vx,
                                                    F* __restrict__ vy, F* __restrict__ vz, RelT* __restrict__ rel) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double tx = W[i], ty = W[fs + i], tz = W[2 * fs + i], xy = W[3 * fs + i], xz = W[4 * fs + i],
                     x2 = W[5 * fs + i], yz = W[6 * fs + i], y2 = W[7 * fs + i], z2 = W[8 * fs + i];
        double ox, oy, oz;
        solve3(x2, y2, z2, xy, xz, yz, tx, ty, tz, ox, oy, oz);
        vx[i] = (F)ox;
        vy[i] = (F)oy;
        vz[i] = (F)oz;
        rel[i] = (RelT)eigmin3<std::is_same_v<RelT, double>>(x2, y2, z2, xy, xz, yz);
    }
}

// 2D (calc_flow.py:154-168). field order: tx ty xy x2 y2
// (grid-stride over a 64-bit count: a 2D batch plan may hold more than 2^31 pixels)
template <typename F>
__global__ __launch_bounds__(256) void k_solve2d(const F* __restrict__ Q, size_t fs, size_t n, F* __restrict__ vx,
                                                 F* __restrict__ vy, F* __restrict__ rel) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double tx = Q[i], ty = Q[fs + i], xy = Q[2 * fs + i], x2 = Q[3 * fs + i], y2 = Q[4 * fs + i];
    const double det = (x2 * y2) - (xy * xy);
    const double R = 1.0 / (det + kEps);
    vx[i] = (F)(R * ((y2 * -tx) + (-xy * -ty)));
    vy[i] = (F)(R * ((-xy * -tx) + (x2 * -ty)));
    const double tr = x2 + y2;
    const double disc = tr * tr - 4.0 * det;
    const double L1 = (tr + sqrt(disc)) / 2.0;
    const double L2 = (tr - sqrt(disc)) / 2.0;
    // np.minimum propagates NaN
    rel[i] = (F)((L1 != L1) ? L1 : ((L2 != L2) ? L2 : (L1 < L2 ? L1 : L2)));
    }
}

// ---------------------------------------------------------------------------
// Downstream statistics (the reference's
// example_analysis_script.ipynb cells 4-6) in one pass over resident outputs:
//   mask = rel > thresh; v = v*mask, v == 0 -> NaN; vx, vy *= xyscale/tscale
//   (as (v*xyscale)/tscale), vz likewise with zscale;
//   magnitude = sqrt((vx*vx + vy*vy) + vz*vz); theta = atan2(vy, vx);
//   phi = atan(vz / sqrt(vx*vx + vy*vy)).  2D: vz == nullptr, no phi.
// ---------------------------------------------------------------------------
template <typename VT, typename RelT>
__global__ __launch_bounds__(256) void k_flow_stats(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                    const VT* __restrict__ vz, const RelT* __restrict__ rel, size_t n,
                                                    double thresh, double sxy, double sz, double st,
                                                    double* __restrict__ ox, double* __restrict__ oy,
                                                    double* __restrict__ oz, double* __restrict__ mag,
                                                    double* __restrict__ theta, double* __restrict__ phi) {
    const size_t stride = (size_t)gridDim.x * 256;
    const double qnan = __builtin_nan("");
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const double m = ((double)rel[i] > thresh) ? 1.0 : 0.0;  // numpy: v * bool mask
        auto fix = [&](double v, double scale) {
            v = v * m;
            if (v == 0.0) v = qnan;
            return (v * scale) / st;
        };
        const double x = fix((double)vx[i], sxy), y = fix((double)vy[i], sxy);
        const double xy2 = x * x + y * y;
        ox[i] = x;
        oy[i] = y;
        theta[i] = atan2(y, x);
        if (vz) {
            const double z = fix((double)vz[i], sz);
            oz[i] = z;
            mag[i] = sqrt(xy2 + z * z);
            phi[i] = atan(z / sqrt(xy2));
        } else {
            mag[i] = sqrt(xy2);
        }
    }
}

}  // namespace

#pragma once
// of3d_k5.hpp — K5: the W z pass + solve + reliability kernels (pipeline overview:
// of3d_common.hpp).
#include <cstdint>
#include <type_traits>

#include "of3d_common.hpp"
#include "of3d_k0.hpp"
#include "of3d_solve.hpp"

namespace {

// K5: W z pass + solve + reliability.  Block = 64 x-columns of one row and
// K5_ZC output planes; per field the (K5_ZC + 2rw)-plane clamped window is
// staged in LDS (double-buffered, next field's loads in flight during this
// field's pass); each thread keeps its K5_R outputs of all 9 fields in
// registers for the pointwise solve.
// Geometry: 64 lanes x G z-groups x R planes per thread (z-block of G*R planes).
// R = 8, G = 8 up to rw 24 (64-plane blocks), else R = 4, G = 8.
struct K5Geom {
    int r, g;
};
constexpr K5Geom k5_geom(int rw) { return {rw <= 24 ? 8 : 4, 8}; }

// Pointwise tail of K5: solve + reliability for the thread's R planes, in
// fp64 whatever the pass type F (fp32 plans solve their float tensor in fp64).
// (K5c: G voxels at a time through solve3 and eigmin3_group — straight-line code, G independent
// chains; the legacy kernels keep G = 1, the same operations per voxel: bit-identical)
template <typename F, typename RelT, int K5_R, int G = 1>
__device__ __forceinline__ void k5_solve_store(const F (&acc)[9][K5_R], int z0l, int nzo, size_t o0, size_t ps,
                                               F* __restrict__ vx, F* __restrict__ vy, F* __restrict__ vz,
                                               RelT* __restrict__ rel) {
    static_assert(K5_R % G == 0, "voxel groups");
    if constexpr (G == 1) {
#pragma unroll
        for (int i = 0; i < K5_R; ++i) {
            if (z0l + i >= nzo) break;
            // field order: tx ty tz xy xz x2 yz y2 z2
            const double tx = acc[0][i], ty = acc[1][i], tz = acc[2][i], xy = acc[3][i], xz = acc[4][i],
                         x2 = acc[5][i], yz = acc[6][i], y2 = acc[7][i], z2 = acc[8][i];
            double ox, oy, oz;
            solve3(x2, y2, z2, xy, xz, yz, tx, ty, tz, ox, oy, oz);
            const size_t o = (size_t)(z0l + i) * ps + o0;
            vx[o] = (F)ox;
            vy[o] = (F)oy;
            vz[o] = (F)oz;
            rel[o] = (RelT)eigmin3<std::is_same_v<RelT, double>>(x2, y2, z2, xy, xz, yz);
        }
    } else {
#pragma unroll
        for (int g0 = 0; g0 < K5_R; g0 += G) {
            if (z0l + g0 >= nzo) break;
            double x2[G], y2[G], z2[G], xy[G], xz[G], yz[G], lam[G];
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int k = g0 + i;
                const double tx = acc[0][k], ty = acc[1][k], tz = acc[2][k];
                xy[i] = acc[3][k], xz[i] = acc[4][k], x2[i] = acc[5][k], yz[i] = acc[6][k], y2[i] = acc[7][k],
                z2[i] = acc[8][k];
                double ox, oy, oz;
                solve3(x2[i], y2[i], z2[i], xy[i], xz[i], yz[i], tx, ty, tz, ox, oy, oz);
                if (z0l + k < nzo) {
                    const size_t o = (size_t)(z0l + k) * ps + o0;
                    vx[o] = (F)ox;
                    vy[o] = (F)oy;
                    vz[o] = (F)oz;
                }
            }
            eigmin3_group<std::is_same_v<RelT, double>, G>(x2, y2, z2, xy, xz, yz, lam);
#pragma unroll
            for (int i = 0; i < G; ++i)
                if (z0l + g0 + i < nzo) rel[(size_t)(z0l + g0 + i) * ps + o0] = (RelT)lam[i];
        }
    }
}

template <typename F, typename RelT, int NJ, int K5_R, int K5_G>
__global__ __launch_bounds__(64 * K5_G) void k_wz_solve(const F* __restrict__ Q, int zq0, int nz, int ny, int nx,
                                                  size_t fs, const F* __restrict__ hw, const F* __restrict__ hwr,
                                                  int rw, int zo0, int nzo, F* __restrict__ vx, F* __restrict__ vy,
                                                  F* __restrict__ vz, RelT* __restrict__ rel) {
    constexpr int K5_ZC = K5_G * K5_R;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* sm = reinterpret_cast<F*>(smem_raw);
    const int H = K5_ZC + 2 * rw;
    const int lane = threadIdx.x, g = threadIdx.y;
    const int x = blockIdx.x * 64 + lane;
    const int xs = x < nx ? x : nx - 1;
    const int y = blockIdx.y;
    const int zc0 = zo0 + blockIdx.z * K5_ZC;
    const size_t ps = (size_t)ny * nx, col = (size_t)y * nx + xs;
    F rq[NJ];
    auto fetch = [&](int f) {
        const F* q = Q + f * fs + col;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int row = g + K5_G * j;
            if (row < H) rq[j] = q[(size_t)(clampi(zc0 - rw + row, 0, nz - 1) - zq0) * ps];
        }
    };
    F acc[9][K5_R];
    fetch(0);
#pragma unroll
    for (int f = 0; f < 9; ++f) {
        F* buf = sm + (f & 1) * H * 64;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int row = g + K5_G * j;
            if (row < H) buf[row * 64 + lane] = rq[j];
        }
        __syncthreads();
        if (f + 1 < 9) fetch(f + 1);
        lds_pass<K5_R, false, false>(buf + lane, 64, rw + g * K5_R, hw, hwr, rw, acc[f]);
    }
    if (x >= nx) return;
    k5_solve_store<F, RelT, K5_R>(acc, zc0 + g * K5_R - zo0, nzo, (size_t)y * nx + x, ps, vx, vy, vz, rel);
}

// Rungs of the runtime-radius kernels: the template instance each getter (kt_*_legacy.hip)
// picks for a radius.  The getters and of3d_plan_geometry's "runtime_radius" both call these,
// so the report cannot drift from the launch.
// k_wz_solve<F, RelT, NJ, R, 8>: NJ rows per thread of the staged window, ceil((G R + 2 rw) / G)
constexpr int k5_nj(int rw) {
    if (k5_geom(rw).r == 8) return rw <= 16 ? 12 : 14;
    const int nj = (8 * 4 + 2 * rw + 7) / 8;
    return nj <= 10 ? 10 : (nj <= 12 ? 12 : 16);
}

// K5 with LDS-DMA staging: the field windows are loaded straight into NB LDS
// buffers, NB - 1 fields ahead of the pass (no staging registers, no VGPR cost
// for the prefetch), so a CU keeps up to (NB - 1) windows of loads in flight
// instead of one field.  One wave-instruction moves 64 lanes x 16 B = RPW rows
// of the 64-column window (RPW = 2 for fp64, 4 for fp32).  Needs nx a
// multiple of 16 B / sizeof(F) (16-byte aligned rows).
// (A persistent form that also prefetches the next tile during the epilogue
// spilled registers and measured slower.)
template <typename F, typename RelT, int NJ2, int K5_R, int K5_G, int NB>
__global__ __launch_bounds__(64 * K5_G) void k_wz_solve_dma(const F* __restrict__ Q, int zq0, int nz, int ny, int nx,
                                                      size_t fs, const F* __restrict__ hw,
                                                      const F* __restrict__ hwr, int rw, int zo0, int nzo,
                                                      F* __restrict__ vx, F* __restrict__ vy, F* __restrict__ vz,
                                                      RelT* __restrict__ rel) {
    constexpr int K5_ZC = K5_G * K5_R;
    constexpr int EPL = 16 / (int)sizeof(F);  // elements per lane per load
    constexpr int RPW = EPL;                  // window rows per wave-instruction
    constexpr int LPR = 64 / RPW;             // lanes per row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* sm = reinterpret_cast<F*>(smem_raw);
    const int H = K5_ZC + 2 * rw;
    const int HG = (H + RPW - 1) / RPW;  // row groups per window
    const int lane = threadIdx.x, g = threadIdx.y;
    const int x = blockIdx.x * 64 + lane;
    const int y = blockIdx.y;
    const int zc0 = zo0 + blockIdx.z * K5_ZC;
    const size_t ps = (size_t)ny * nx;
    const int xc = min((int)blockIdx.x * 64 + EPL * (lane % LPR), nx - EPL);  // this lane's columns
    const F* qrow = Q + (size_t)y * nx + xc;
    const unsigned lds0 = (unsigned)(uintptr_t)smem_raw;
    auto issue = [&](int f, int b) {
        const F* q = qrow + f * fs;
        const unsigned lb = lds0 + (unsigned)(b * HG * 1024);
#pragma unroll
        for (int j = 0; j < NJ2; ++j) {
            const int p = min(g + K5_G * j, HG - 1);  // surplus slots repeat the last group: equal counts per wave
            const int row = min(RPW * p + lane / LPR, H - 1);
            const F* src = q + (size_t)(clampi(zc0 - rw + row, 0, nz - 1) - zq0) * ps;
            glds16(src, __builtin_amdgcn_readfirstlane(lb + (unsigned)(p * 1024)));
        }
    };
    F acc[9][K5_R];
#pragma unroll
    for (int f = 0; f < NB - 1; ++f) issue(f, f);
#pragma unroll
    for (int f = 0; f < 9; ++f) {
        // field f landed (loads of the fields issued after it may stay in flight: loads
        // retire in issue order), and every wave is done reading the buffer the next
        // issue overwrites
        const int ahead = min(NB - 2, 8 - f);
        if (ahead >= 2)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * NJ2) : "memory");
        else if (ahead == 1)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(NJ2) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (f + NB - 1 < 9) issue(f + NB - 1, (f + NB - 1) % NB);
        lds_pass<K5_R, false>(sm + (f % NB) * HG * RPW * 64 + lane, 64, rw + g * K5_R, hw, hwr, rw, acc[f]);
    }
    if (x >= nx) return;
    k5_solve_store<F, RelT, K5_R>(acc, zc0 + g * K5_R - zo0, nzo, (size_t)y * nx + x, ps, vx, vy, vz, rel);
}

// LDS-DMA K5: NB window buffers of ceil(H / RPW) 1-KB row groups (RPW = 16 B /
// sizeof(F) rows); NJ2 = groups per wave.
template <typename F>
constexpr int k5_groups(int rw) {
    constexpr int rpw = 16 / (int)sizeof(F);
    return (k5_geom(rw).g * k5_geom(rw).r + 2 * rw + rpw - 1) / rpw;
}
template <typename F>
int k5_dma_nb(int rw) {
    const size_t buf = (size_t)k5_groups<F>(rw) * 1024, lim = 160 * 1024;
    return 3 * buf <= lim ? 3 : (2 * buf <= lim ? 2 : 0);
}
// k_wz_solve_dma<F, RelT, NJ2, R, 8, NB>: NJ2 row groups per wave (fp64: <= 7 for rw <= 24,
// <= 8 for rw <= 48; fp32: <= 4)
template <typename F>
constexpr int k5_dma_nj2(int rw) {
    const K5Geom k = k5_geom(rw);
    const int nj2 = (k5_groups<F>(rw) + k.g - 1) / k.g;
    if constexpr (sizeof(F) == 8) {
        if (k.r == 8) return nj2 <= 6 ? 6 : 7;
        return nj2 <= 6 ? 6 : (nj2 <= 7 ? 7 : 8);
    } else {
        return nj2 <= 3 ? 3 : 4;
    }
}

// voxels per straight-line group in K5c's epilogue (k5_solve_store): 4 in fp64 (206 VGPRs either
// way, set by the nine fields' accumulators); 1 in fp32, where the four voxels' fp64 epilogue state
// took the kernel from 112 to 158 VGPRs, 4 -> 3 waves per SIMD — the round-4/5 c5 regression (same
// box, round-3 tree vs round-6: K5c 35.1 vs 36.6 ms, profiles/r06/ab_c5_r03/; G 1 vs 4 on one box:
// K5c 35.3 / 35.2 vs 36.6 / 36.7 ms, frame 102.8 / 102.9 vs 104.0 / 104.4, profiles/r06/ab6/c5_*)
template <typename F>
constexpr int K5C_G = sizeof(F) == 8 ? 4 : 1;
// LDS-read distance of K5c's W z passes (lds_pass_c's D: window values read D taps ahead).  fp64:
// 3 (c3 K5c 0.993 / 0.994 -> 0.979 / 0.974 ms over four same-box pairs, c4 6.80 -> 6.75; 4: c3
// 0.98, c4 slower; the VGPR count stays 206, set by the epilogue); fp32 keeps 2 (c5: 36.0 vs
// 36.1 ms).  profiles/r05/ab_k5c_d/
template <typename F>
constexpr int K5C_D = sizeof(F) == 8 ? 3 : 2;

// K5c block coordinates from the launch's (columns, rows, z chunks) grid, XCD-aware: the
// linear workgroup id b runs on XCD b % 8, so the z chunks of one (column block, row) — whose
// windows share 2 rw W-xy planes — get ids 8 apart (same XCD, dispatched back to back) and
// the shared planes come from that XCD's L2 instead of HBM twice.  A bijection on the grid
// (the tail past the last whole group of 8 z-chunk sets keeps the plain order).
struct K5Block {
    int bx, by, bz;
};
__device__ __forceinline__ K5Block k5c_block() {
    if (gridDim.z == 1) return {(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
    const unsigned gx = gridDim.x, gxy = gx * gridDim.y, nz = gridDim.z;
    const unsigned b = blockIdx.x + gx * (blockIdx.y + gridDim.y * blockIdx.z);
    const unsigned full = (gxy * nz) / (8 * nz) * (8 * nz);
    unsigned rest, zc;
    if (b < full) {
        const unsigned j = b >> 3;
        zc = j % nz;
        rest = (j / nz) * 8 + (b & 7);
    } else {
        const unsigned l = b - full;
        zc = l % nz;
        rest = full / nz + l / nz;
    }
    return {(int)(rest % gx), (int)(rest / gx), (int)zc};
}

// K5c: the LDS-DMA W z + solve with a compile-time window radius (taps in SGPRs,
// lds_pass_c: no weight loads or waits inside the passes) and narrow blocks: CB = 32
// columns x 2 z-groups per wave, 4 waves (256 threads), R planes per z-group, so a
// block holds ZC = 8 R output planes of 32 columns and its window of ZC + 2RW planes
// per field takes NB buffers of HG 1-KiB row groups (fp64, RW 15: 24 KiB each).  Two
// blocks fit a CU: one block's prologue / epilogue overlaps another's passes.
// RT0 > 0: after its solve, every block also forms its share of the next frame's dt0 (K0Next,
// input type T0): a contiguous range of voxel groups per block, the K0c arithmetic (k0_group).
template <typename F, typename RelT, int RW, int NB, int R, int NW = 4, int RT0 = 0, typename T0 = uint16_t>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 1 : (R == 8 ? 2 : 3)) void k_wz_solve_c(
    const F* __restrict__ Q, int zq0, int nz, int ny, int nx, size_t fs, const F* __restrict__ hw, int zo0, int nzo,
    F* __restrict__ vx, F* __restrict__ vy, F* __restrict__ vz, RelT* __restrict__ rel, int yo0, K0Next<F> k0, int zt) {
    // NW 8: 128-plane blocks (one per CU), window 1.33x the output planes instead of 1.66x
    constexpr int CB = 32, LPC = 64 / CB;  // columns per block, z-groups per wave
    constexpr int ZC = NW * LPC * R;                // output planes per block (R planes per z-group)
    constexpr int H = ZC + 2 * RW;                  // window rows (planes)
    constexpr int EPL = 16 / (int)sizeof(F);        // elements per lane per DMA
    constexpr int LPR = CB / EPL;                   // lanes per window row
    constexpr int RPWI = 64 / LPR;                  // window rows per wave-instruction (1 KiB)
    constexpr int HG = (H + RPWI - 1) / RPWI;       // row groups per window
    constexpr int NJ2 = (HG + NW - 1) / NW;         // row groups per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* sm = reinterpret_cast<F*>(smem_raw);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane % CB, gz = w * LPC + lane / CB;
    const K5Block kb = k5c_block();
    const int x = kb.bx * CB + col;
    const int y = yo0 + kb.by;  // outputs: rows [yo0, yo0 + gridDim.y) in a compact layout
    const int zc0 = zo0 + kb.bz * ZC;
    const size_t ps = (size_t)ny * nx;
    const int xc = min(kb.bx * CB + EPL * (lane % LPR), nx - EPL);  // this lane's DMA columns
    // the window column of this lane: plane-major rows (zt == 0) or one z-tiled run (zt > 0, nx a
    // multiple of 32: xc & 31 is the lane's column in the tile)
    const F* qrow = zt ? Q + ((size_t)y * (nx >> 5) + (xc >> 5)) * zt * 32 + (xc & 31) : Q + (size_t)y * nx + xc;
    const size_t zs = zt ? 32 : ps;  // element stride of one window plane
    const unsigned lds0 = (unsigned)(uintptr_t)smem_raw;
    F h[RW + 1];
#pragma unroll
    for (int k = 0; k <= RW; ++k) h[k] = hw[k];
    auto issue = [&](int f, int b) {
        const F* q = qrow + f * fs;
        const unsigned lb = lds0 + (unsigned)(b * HG * 1024);
#pragma unroll
        for (int j = 0; j < NJ2; ++j) {
            const int pg = min(w + NW * j, HG - 1);  // surplus slots repeat the last group: equal counts per wave
            const int row = min(RPWI * pg + lane / LPR, H - 1);
            const F* src = q + (size_t)(clampi(zc0 - RW + row, 0, nz - 1) - zq0) * zs;
            glds16(src, __builtin_amdgcn_readfirstlane(lb + (unsigned)(pg * 1024)));
        }
    };
    F acc[9][R];
#pragma unroll
    for (int f = 0; f < NB - 1; ++f) issue(f, f);
    // RT0 > 0: the next frame's dt0 for this block's first groups, loaded right behind the
    // first field's DMA (the two latencies overlap) and held to the end (stores after the solve)
    constexpr int V0 = K0Vec<T0>::V, NG0 = RT0 > 0 ? 2 : 0;
    F dtn[NG0 > 0 ? NG0 : 1][V0];
    size_t k0g0 = 0, k0g1 = 0;
    if constexpr (RT0 > 0) {
        const size_t nblk = (size_t)gridDim.x * gridDim.y * gridDim.z;
        const size_t lin = blockIdx.x + (size_t)gridDim.x * (blockIdx.y + (size_t)gridDim.y * blockIdx.z);
        const size_t per = (k0.ngroups + nblk - 1) / nblk;
        k0g0 = lin * per;
        k0g1 = min(k0g0 + per, k0.ngroups);
        F h0[RT0 + 1];
#pragma unroll
        for (int k = 0; k <= RT0; ++k) h0[k] = k0.ht[k];
#pragma unroll
        for (int j = 0; j < NG0; ++j) {
            const size_t gi = k0g0 + threadIdx.x + (size_t)j * 64 * NW;
            if (gi < k0g1) k0_group_dt<T0, F, RT0>(k0.fr, k0.off0 + gi * V0, h0, dtn[j]);
        }
    }
#pragma unroll
    for (int f = 0; f < 9; ++f) {
        // as k_wz_solve_dma: field f landed, the buffer the next issue overwrites is free
        const int ahead = min(NB - 2, 8 - f);
        if (ahead >= 2)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * NJ2) : "memory");
        else if (ahead == 1)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(NJ2) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (f + NB - 1 < 9) issue(f + NB - 1, (f + NB - 1) % NB);
        lds_pass_c<R, RW, K5C_D<F>, false, k5c_solo<F>>(sm + (f % NB) * HG * RPWI * CB + col, CB, RW + gz * R, h,
                                                    acc[f]);
        // pin the pass here: without it the compiler sinks every field's arithmetic below the
        // last barrier and keeps all 9 windows' LDS reads live in registers (spills)
#pragma unroll
        for (int i = 0; i < R; ++i) asm volatile("" : "+v"(acc[f][i]));
    }
    if (x < nx)
        k5_solve_store<F, RelT, R, K5C_G<F>>(acc, zc0 + gz * R - zo0, nzo, (size_t)kb.by * nx + x, (size_t)gridDim.y * nx, vx,
                                   vy, vz, rel);
    if constexpr (RT0 > 0) {  // the next frame's dt0: the held groups, then any rest of [k0g0, k0g1)
#pragma unroll
        for (int j = 0; j < NG0; ++j) {
            const size_t gi = k0g0 + threadIdx.x + (size_t)j * 64 * NW;
            if (gi < k0g1) k0_store<F, V0>(dtn[j], k0.D0 + gi * V0);
        }
        F h0[RT0 + 1];
#pragma unroll
        for (int k = 0; k <= RT0; ++k) h0[k] = k0.ht[k];
        for (size_t gi = k0g0 + threadIdx.x + (size_t)NG0 * 64 * NW; gi < k0g1; gi += 64 * NW)
            k0_group<T0, F, RT0>(k0.fr, k0.off0 + gi * V0, h0, k0.D0 + gi * V0);
    }
}
constexpr int k5c_zc(int r, int nw = 4) { return 2 * nw * r; }  // output planes per K5c block (R per z-group)
template <typename F>
constexpr int k5c_groups(int rw, int r, int nw = 4) {
    constexpr int rpwi = 64 / (32 / (16 / (int)sizeof(F)));
    return (k5c_zc(r, nw) + 2 * rw + rpwi - 1) / rpwi;
}

}  // namespace

#pragma once
// of3d_grad.hpp — the gradient passes as separate kernels: K1 / K2 (runtime radius) and the
// column marches K1c / K2c (pipeline overview: of3d_common.hpp).
#include <utility>

#include "of3d_common.hpp"

namespace {

// ---------------------------------------------------------------------------
// K1: y and x passes of the gradient filters (calc_flow.py:279-288, y first):
//   A1 = y(G)[dt0], A2 = y(D)[I], A3 = y(S)[I]
//   B1 = x(G)[A1] (dt), B2 = x(S)[A2] (dy), B3 = x(D)[A3] (dx), B4 = x(S)[A3] (dz)
// Block = one 64-wide staged column strip (64 - 2rd output columns) x K1_TY
// output rows, walking K1_NZB planes; lane = staged column.  The next plane's
// I / dt0 rows are fetched into registers during this plane's passes.  The y
// pass is a ring pass down each lane's column; the x pass reads neighbour
// columns from LDS.
// ---------------------------------------------------------------------------
constexpr int K1_R = 4, K1_TY = 4 * K1_R, K1_NZB = 4;

template <typename T, typename F, int NJ>
__global__ __launch_bounds__(256, 3) void k_grad_xy(const T* __restrict__ Ic, const F* __restrict__ D0, int ny,
                                                 int nx, int nzp, DevTaps<F> tp, F* __restrict__ B, size_t fs,
                                                 int need_b4) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* smem = reinterpret_cast<F*>(smem_raw);
    const int rd = tp.rd, rs = tp.rs;
    const int RH = K1_TY + 2 * rd;
    F* sI = smem;
    F* sT = sI + RH * 64;
    F* sA1 = sT + RH * 64;
    F* sA2 = sA1 + K1_TY * 64;
    F* sA3 = sA2 + K1_TY * 64;
    const int lane = threadIdx.x, w = threadIdx.y;
    const int x0 = blockIdx.x * (64 - 2 * rd), y0 = blockIdx.y * K1_TY;
    const int zb = blockIdx.z * K1_NZB;
    const int nzb = min(K1_NZB, nzp - zb);
    const size_t ps = (size_t)ny * nx;
    const int gx = clampi(x0 - rd + lane, 0, nx - 1);
    int roff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) roff[j] = clampi(y0 - rd + w + 4 * j, 0, ny - 1) * nx + gx;
    F rI[NJ], rT[NJ];
    auto fetch = [&](int t) {
        const T* ip = Ic + (size_t)(zb + t) * ps;
        const F* dp = D0 + (size_t)(zb + t) * ps;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (w + 4 * j < RH) {
                rI[j] = (F)ip[roff[j]];
                rT[j] = dp[roff[j]];
            }
    };
    fetch(0);
    const int gxo = x0 + lane - rd;
    const bool xout = lane >= rd && lane < 64 - rd && gxo < nx;
    for (int t = 0; t < nzb; ++t) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int row = w + 4 * j;
            if (row < RH) {
                sI[row * 64 + lane] = rI[j];
                sT[row * 64 + lane] = rT[j];
            }
        }
        __syncthreads();
        if (t + 1 < nzb) fetch(t + 1);
        {
            F a[K1_R];
            const int base = rd + w * K1_R;
            lds_pass<K1_R, false, false>(sT + lane, 64, base, tp.g, tp.gr, rd, a);
#pragma unroll
            for (int i = 0; i < K1_R; ++i) sA1[(w * K1_R + i) * 64 + lane] = a[i];
            lds_pass<K1_R, true, false>(sI + lane, 64, base, tp.d, tp.dr, rd, a);
#pragma unroll
            for (int i = 0; i < K1_R; ++i) sA2[(w * K1_R + i) * 64 + lane] = a[i];
            lds_pass<K1_R, false, false>(sI + lane, 64, base, tp.s, tp.sr, rs, a);
#pragma unroll
            for (int i = 0; i < K1_R; ++i) sA3[(w * K1_R + i) * 64 + lane] = a[i];
        }
        __syncthreads();
        if (xout) {
            F* bp = B + (size_t)(zb + t) * ps + gxo;
#pragma unroll
            for (int i = 0; i < K1_R; ++i) {
                const int row = w * K1_R + i;
                const int gy = y0 + row;
                if (gy >= ny) break;
                const int c = row * 64 + lane;
                F b1 = sA1[c] * tp.g[0], b2 = sA2[c] * tp.s[0], b3 = sA3[c] * tp.d[0], b4 = sA3[c] * tp.s[0];
                for (int k = rd; k >= 1; --k) {
                    b1 = b1 + (sA1[c - k] + sA1[c + k]) * tp.g[k];
                    b3 = b3 + (sA3[c - k] - sA3[c + k]) * tp.d[k];
                }
                for (int k = rs; k >= 1; --k) {
                    b2 = b2 + (sA2[c - k] + sA2[c + k]) * tp.s[k];
                    b4 = b4 + (sA3[c - k] + sA3[c + k]) * tp.s[k];
                }
                const size_t o = (size_t)gy * nx;
                bp[o] = b1;
                bp[fs + o] = b2;
                bp[2 * fs + o] = b3;
                if (need_b4) bp[3 * fs + o] = b4;
            }
        }
        __syncthreads();
    }
}

// Rungs of the runtime-radius kernels: the template instance each getter (kt_*_legacy.hip)
// picks for a radius.  The getters and of3d_plan_geometry's "runtime_radius" both call these,
// so the report cannot drift from the launch.
// k_grad_xy<T, F, NJ>: NJ rows per thread of the (K1_TY + 2 rd)-row staged strip, 4 waves
constexpr int k1_nj(int rd) {
    const int nj = (K1_TY + 2 * rd + 3) / 4;
    return nj <= 8 ? 8 : (nj <= 12 ? 12 : 16);
}

// ---------------------------------------------------------------------------
// K2: z pass of the gradients (calc_flow.py:279-288, last pass, axis 0):
//   dt = z(G)[B1], dy = z(S)[B2], dx = z(S)[B3], dz = z(D)[B4]
// One field per block: 64 x-columns of one row, K2_ZC output planes; the
// (K2_ZC + 2r)-plane clamped window is staged in LDS, ring pass per lane.
// ---------------------------------------------------------------------------
constexpr int K2_R = 4, K2_ZC = 4 * K2_R;

template <typename F>
__global__ __launch_bounds__(256) void k_grad_z(const F* __restrict__ B, int zb0, F* __restrict__ G, int zg0, int nzg,
                                                int nz, int ny, int nx, size_t fs, DevTaps<F> tp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* sm = reinterpret_cast<F*>(smem_raw);
    const int f = blockIdx.z & 3;
    const int zc = blockIdx.z >> 2;
    const F* h = f == 0 ? tp.g : (f == 3 ? tp.d : tp.s);
    const F* hr = f == 0 ? tp.gr : (f == 3 ? tp.dr : tp.sr);
    const int r = (f == 0 || f == 3) ? tp.rd : tp.rs;
    const int H = K2_ZC + 2 * r;
    const int lane = threadIdx.x, g = threadIdx.y;
    const int x = blockIdx.x * 64 + lane;
    const int xs = x < nx ? x : nx - 1;
    const int y = blockIdx.y;
    const int zc0 = zg0 + zc * K2_ZC;
    const size_t ps = (size_t)ny * nx, col = (size_t)y * nx + xs;
    const F* src = B + f * fs + col;
    for (int row = g; row < H; row += 4)
        sm[row * 64 + lane] = src[(size_t)(clampi(zc0 - r + row, 0, nz - 1) - zb0) * ps];
    __syncthreads();
    F out[K2_R];
    if (f == 3)
        lds_pass<K2_R, true>(sm + lane, 64, r + g * K2_R, h, hr, r, out);
    else
        lds_pass<K2_R, false>(sm + lane, 64, r + g * K2_R, h, hr, r, out);
    if (x >= nx) return;
    F* dst = G + f * fs + (size_t)y * nx + x;
#pragma unroll
    for (int i = 0; i < K2_R; ++i) {
        const int zl = zc0 + g * K2_R + i - zg0;
        if (zl < nzg) dst[(size_t)zl * ps] = out[i];
    }
}

// ---------------------------------------------------------------------------
// K2c: the gradient z pass (calc_flow.py:279-288, axis 0) as a z march: thread = one
// (y, x) column, lanes along x (coalesced), marching a chunk of zc output planes with a
// register ring of NR planes per field (compile-time slots, as K34); no LDS, no
// barriers, every input plane read once per chunk.  dt = z(G)[B1], dy = z(S)[B2],
// dx = z(S)[B3], dz = z(D)[B4], same order as k_grad_z: bit-identical.
// ---------------------------------------------------------------------------
template <typename F, int RD, int RS>
__global__ __launch_bounds__(256, 3) void k_grad_z_c(const F* __restrict__ B, int zb0, F* __restrict__ G, int zg0,
                                                     int nzg, int nz, int plane, size_t fs, DevTaps<F> tp, int zc) {
    constexpr int NR = ((2 * RD + 2 + 7) / 8) * 8, PD = 4;
    static_assert(NR % PD == 0 && RS <= RD, "ring sizes");
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= plane) return;
    const int zc0 = zg0 + blockIdx.y * zc;
    const int nrows = min(zc, zg0 + nzg - zc0);
    F hg[RD + 1], hd[RD + 1], hs[RS + 1];
#pragma unroll
    for (int k = 0; k <= RD; ++k) hg[k] = tp.g[k], hd[k] = tp.d[k];
#pragma unroll
    for (int k = 0; k <= RS; ++k) hs[k] = tp.s[k];
    const F* b = B + col;
    F* g = G + col;
    auto src = [&](int idx) { return (size_t)(clampi(zc0 - RD + idx, 0, nz - 1) - zb0) * plane; };
    F ring[4][NR], raw[4][PD];
#pragma unroll
    for (int i = 0; i <= 2 * RD; ++i) {
        const size_t o = src(i);
#pragma unroll
        for (int f = 0; f < 4; ++f) ring[f][i] = b[f * fs + o];
    }
#pragma unroll
    for (int i = 0; i < PD; ++i) {
        const size_t o = src(2 * RD + 1 + i);
#pragma unroll
        for (int f = 0; f < 4; ++f) raw[f][(2 * RD + 1 + i) % PD] = b[f * fs + o];
    }
    for (int u0 = 0; u0 < nrows; u0 += NR) {
        bool done = false;
        [&]<int... J>(std::integer_sequence<int, J...>) {
            (
                [&] {
                    if (done) return;
                    constexpr int j = J;
                    constexpr int ic = j + 2 * RD + 1, c = (j + RD) % NR;
                    const size_t o = src(u0 + ic + PD);
#pragma unroll
                    for (int f = 0; f < 4; ++f) {
                        ring[f][ic % NR] = raw[f][ic % PD];
                        raw[f][ic % PD] = b[f * fs + o];
                    }
                    F o0 = ring[0][c] * hg[0], o3 = ring[3][c] * hd[0];
                    F o1 = ring[1][c] * hs[0], o2 = ring[2][c] * hs[0];
#pragma unroll
                    for (int k = RD; k >= 1; --k) {
                        o0 = o0 + (ring[0][(j + RD - k) % NR] + ring[0][(j + RD + k) % NR]) * hg[k];
                        o3 = o3 + (ring[3][(j + RD - k) % NR] - ring[3][(j + RD + k) % NR]) * hd[k];
                    }
#pragma unroll
                    for (int k = RS; k >= 1; --k) {
                        o1 = o1 + (ring[1][(j + RD - k) % NR] + ring[1][(j + RD + k) % NR]) * hs[k];
                        o2 = o2 + (ring[2][(j + RD - k) % NR] + ring[2][(j + RD + k) % NR]) * hs[k];
                    }
                    const size_t d = (size_t)(zc0 + u0 + j - zg0) * plane;
                    g[d] = o0;
                    g[fs + d] = o1;
                    g[2 * fs + d] = o2;
                    g[3 * fs + d] = o3;
                    if (u0 + j + 1 >= nrows) done = true;
                }(),
                ...);
        }(std::make_integer_sequence<int, NR>{});
        if (done) break;
    }
}

// ---------------------------------------------------------------------------
// K1c: K1 as a column march (the K34 scheme, calc_flow.py:279-288 y and x passes):
// thread = staged column of one plane (RD halo columns each side), marching its rows.
// Register rings of the centre frame I and of dt0 (NR rows, compile-time slots) give
// the y passes A1 = y(G)[dt0], A2 = y(D)[I], A3 = y(S)[I] with no LDS reads; each row
// lands in three LDS tiles (double-buffered, S rows).  Every S rows the x passes
// B1 = x(G)[A1] (dt), B2 = x(S)[A2] (dy), B3 = x(D)[A3] (dx), B4 = x(S)[A3] (dz)
// run over the tile with lds_pass_c (same item -> lane map as k_prod_wyx) and store
// from registers.  Same expression order as k_grad_xy: bit-identical.
// ---------------------------------------------------------------------------
constexpr int K1C_S = 4;

template <typename T, typename F, int RD, int RS, int S>
__global__ __launch_bounds__(256, 3) void k_grad_xy_c(const T* __restrict__ Ic, const F* __restrict__ D0, int ny,
                                                      int nx, DevTaps<F> tp, F* __restrict__ B, size_t fs,
                                                      int need_b4, int tx, int nyc, int nbx, int nyb) {
    constexpr int NR = ((2 * RD + 2 + S - 1) / S) * S;
    constexpr int PD = NR % 8 == 0 ? 8 : 4;
    constexpr int RB = 4;
    constexpr unsigned ES = sizeof(F);
    static_assert(NR % PD == 0 && NR % S == 0 && RS <= RD, "ring sizes");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* sm = reinterpret_cast<F*>(smem_raw);  // [2 buffers][3 tiles][k34_tile(S, cwp)]
    const int cw = blockDim.x, cwp = cw + 1, tl = k34_tile(S, cwp);
    const int t = threadIdx.x;
    int b = blockIdx.x;
    const int bx = b % nbx;
    b /= nbx;
    const int yc = b % nyb, z = b / nyb;
    const int y0 = yc * nyc, nrows = min(nyc, ny - y0);
    const int xo0 = bx * tx;
    const int txu = min(tx, nx - xo0);
    const int wa = (min(cw, txu + 2 * RD) + 63) >> 6, ca = 64 * wa;
    if (t >= ca) return;
    const size_t ps = (size_t)ny * nx;
    const unsigned gx = (unsigned)clampi(xo0 - RD + t, 0, nx - 1);
    const auto ri_ = buf_rsrc(Ic + (size_t)z * ps);
    const auto rt_ = buf_rsrc(D0 + (size_t)z * ps);
    F* bz = B + (size_t)z * ps + xo0;
    const auto rb0 = buf_rsrc(bz), rb1 = buf_rsrc(bz + fs), rb2 = buf_rsrc(bz + 2 * fs), rb3 = buf_rsrc(bz + 3 * fs);
    F hg[RD + 1], hd[RD + 1], hs[RS + 1];
#pragma unroll
    for (int k = 0; k <= RD; ++k) hg[k] = tp.g[k], hd[k] = tp.d[k];
#pragma unroll
    for (int k = 0; k <= RS; ++k) hs[k] = tp.s[k];
    auto row = [&](int idx) { return (unsigned)clampi(y0 - RD + idx, 0, ny - 1) * (unsigned)nx; };
    F ri[NR], rt[NR], pt[PD];
    T pi[PD];
#pragma unroll
    for (int i = 0; i <= 2 * RD; ++i) {
        const unsigned o = row(i);
        ri[i] = (F)buf_ld_raw<T>(ri_, gx * (unsigned)sizeof(T), o * (unsigned)sizeof(T));
        rt[i] = buf_ld<F>(rt_, gx * ES, o * ES);
    }
#pragma unroll
    for (int i = 0; i < PD; ++i) {
        const unsigned o = row(2 * RD + 1 + i);
        pi[(2 * RD + 1 + i) % PD] = buf_ld_raw<T>(ri_, gx * (unsigned)sizeof(T), o * (unsigned)sizeof(T));
        pt[(2 * RD + 1 + i) % PD] = buf_ld<F>(rt_, gx * ES, o * ES);
    }
    const int nseg = (txu + RB - 1) / RB;
    constexpr int RPW = S < 8 ? S : 8, SPW = 64 / RPW, RG = S / RPW;
    const int nsgw = (nseg + SPW - 1) / SPW;
    const unsigned rowb = (unsigned)nx * ES;
    auto store = [&](const F (&v)[RB], __amdgpu_buffer_rsrc_t rs, unsigned vo, int c0) {
        if (c0 + RB <= txu) {
            buf_st_n<F, RB>(v, rs, vo, 0);
        } else {
            for (int e = 0; e < RB; ++e)
                if (c0 + e < txu) buf_st<F>(v[e], rs, vo + e * ES, 0);
        }
    };
    auto phase_b = [&](const F* tiles, int yb, int nr) {
        lds_barrier();
        for (int i = t; i < 64 * RG * nsgw; i += ca) {
            const int l = i & 63, wg = i >> 6;
            const int r = (wg % RG) * RPW + ((l >> 2) & 3) + (S >= 8 ? 4 * (l >> 5) : 0);
            const int sg = (wg / RG) * SPW + (l & 3) + 4 * ((l >> 4) & 1) + (S >= 8 ? 0 : 8 * (l >> 5));
            if (sg >= nseg || r >= nr) continue;
            const int c0 = RB * sg, base = RD + RB * sg;
            const unsigned vo = (unsigned)(yb + r) * rowb + (unsigned)c0 * ES;
            const int ro = k34_row(r, cwp);
            F o[RB];
            lds_pass_c<RB, RD, 2>(tiles + ro, 1, base, hg, o);  // dt
            store(o, rb0, vo, c0);
            lds_pass_c<RB, RS, 2>(tiles + tl + ro, 1, base, hs, o);  // dy
            store(o, rb1, vo, c0);
            lds_pass_c<RB, RD, 2, true>(tiles + 2 * tl + ro, 1, base, hd, o);  // dx
            store(o, rb2, vo, c0);
            if (need_b4) {
                lds_pass_c<RB, RS, 2>(tiles + 2 * tl + ro, 1, base, hs, o);  // dz (pre-z)
                store(o, rb3, vo, c0);
            }
        }
    };
    for (int u0 = 0; u0 < nrows; u0 += NR) {
        bool done = false;
        [&]<int... H>(std::integer_sequence<int, H...>) {
            (
                [&] {
                    if (done) return;
                    constexpr int h0 = H * S;
                    F* tiles = sm + (((u0 + h0) / S) & 1) * (3 * tl);
                    [&]<int... J>(std::integer_sequence<int, J...>) {
                        (
                            [&] {
                                constexpr int j = h0 + J;
                                constexpr int ic = j + 2 * RD + 1;
                                ri[ic % NR] = (F)pi[ic % PD];
                                rt[ic % NR] = pt[ic % PD];
                                const unsigned o = row(u0 + ic + PD);
                                pi[ic % PD] = buf_ld_raw<T>(ri_, gx * (unsigned)sizeof(T), o * (unsigned)sizeof(T));
                                pt[ic % PD] = buf_ld<F>(rt_, gx * ES, o * ES);
                                constexpr int c = (j + RD) % NR;
                                F a1 = rt[c] * hg[0], a2 = ri[c] * hd[0], a3 = ri[c] * hs[0];
#pragma unroll
                                for (int k = RD; k >= 1; --k) {
                                    a1 = a1 + (rt[(j + RD - k) % NR] + rt[(j + RD + k) % NR]) * hg[k];
                                    a2 = a2 + (ri[(j + RD - k) % NR] - ri[(j + RD + k) % NR]) * hd[k];
                                }
#pragma unroll
                                for (int k = RS; k >= 1; --k)
                                    a3 = a3 + (ri[(j + RD - k) % NR] + ri[(j + RD + k) % NR]) * hs[k];
                                const int ro = k34_row(j % S, cwp) + t;
                                tiles[ro] = a1;
                                tiles[tl + ro] = a2;
                                tiles[2 * tl + ro] = a3;
                            }(),
                            ...);
                    }(std::make_integer_sequence<int, S>{});
                    const int yb = u0 + h0;
                    phase_b(tiles, y0 + yb, min(S, nrows - yb));
                    if (yb + S >= nrows) done = true;
                }(),
                ...);
        }(std::make_integer_sequence<int, NR / S>{});
        if (done) break;
    }
}

}  // namespace

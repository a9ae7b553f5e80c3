#pragma once
// of3d_k34.hpp — the structure-tensor products and the W y / W x passes: K3 and K4 (runtime
// radius) and the three fused K34 kernels (pipeline overview: of3d_common.hpp).
#include <utility>

#include "of3d_common.hpp"

namespace {

// ---------------------------------------------------------------------------
// K3: structure-tensor products + W y pass (calc_flow.py:300-313; 2D :133-141).
// Gradient field index: 0 dt, 1 dy, 2 dx, 3 dz.
// 3D product order: tx ty tz xy xz x2 yz y2 z2 ;  2D: tx ty xy x2 y2.
// Block = 64 x-columns x K3_YC rows of one plane.  Per product: the product
// over the (K3_YC + 2rw)-row clamped halo is staged in LDS (double-buffered;
// the next product's gradient loads are in flight during this product's
// pass), then each thread produces K3_R rows by a register-rotated window.
// ---------------------------------------------------------------------------
constexpr int K3_R = 8, K3_YC = 4 * K3_R;

// Streaming form: a block owns one 64-column strip of one plane and one
// product, and marches down the whole column height K3_STEP rows at a time.
// The LDS window holds rows y' = y0 .. y0 + K3_STEP + 2rw - 1 (y' = y + rw);
// after each step its last 2rw rows move to the front (so every row is
// loaded from memory once, and every tap read is a constant LDS offset); the
// next step's rows are fetched into registers during the current pass.
constexpr int K3_STEP = K3_YC;

template <typename F, int NP, int TJ>  // TJ >= ceil(2rw / 4): window rows each thread carries over
__global__ __launch_bounds__(256) void k_prod_wy(const F* __restrict__ G, F* __restrict__ P, int ny, int nx,
                                                 size_t fs, const F* __restrict__ hw, const F* __restrict__ hwr,
                                                 int rw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* sm = reinterpret_cast<F*>(smem_raw);
    constexpr int NJ = K3_STEP / 4;  // new rows per thread per step
    const int lane = threadIdx.x, g = threadIdx.y;
    const int x = blockIdx.x * 64 + lane;
    const int xs = x < nx ? x : nx - 1;
    const int p = blockIdx.z % NP;
    const size_t pl = (size_t)(blockIdx.z / NP) * ny * nx;
    // packed product table (4 bits per entry)
    constexpr unsigned long long pa = NP == 9 ? 0x311222312ull : 0x12212ull;  // a[] = {2,1,3,2,2,2,1,1,3} / {2,1,2,2,1}
    constexpr unsigned long long pb = NP == 9 ? 0x313231000ull : 0x12100ull;  // b[] = {0,0,0,1,3,2,3,1,3} / {0,0,1,2,1}
    const F* ga = G + (size_t)((pa >> (4 * p)) & 15u) * fs + pl + xs;
    const F* gb = G + (size_t)((pb >> (4 * p)) & 15u) * fs + pl + xs;
    const int h2 = 2 * rw;
    F* col = sm + lane;
    for (int b = g; b < h2; b += 4) {  // prologue: y' in [0, 2rw)
        const size_t o = (size_t)clampi(b - rw, 0, ny - 1) * nx;
        col[b * 64] = ga[o] * gb[o];
    }
    F ra[NJ], rb[NJ];
    auto fetch = [&](int yp0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const size_t o = (size_t)clampi(yp0 + g + 4 * j - rw, 0, ny - 1) * nx;
            ra[j] = ga[o];
            rb[j] = gb[o];
        }
    };
    fetch(h2);
    F* o = P + p * fs + pl + x;
    F tl[TJ];
    for (int y0 = 0; y0 < ny; y0 += K3_STEP) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) col[(h2 + g + 4 * j) * 64] = ra[j] * rb[j];
        __syncthreads();
        const bool more = y0 + K3_STEP < ny;
        if (more) fetch(y0 + K3_STEP + h2);
        F out[K3_R];
        lds_pass<K3_R, false, (TJ <= 8)>(col, 64, rw + g * K3_R, hw, hwr, rw, out);
        if (x < nx) {
#pragma unroll
            for (int i = 0; i < K3_R; ++i) {
                const int y = y0 + g * K3_R + i;
                if (y < ny) o[(size_t)y * nx] = out[i];
            }
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < TJ; ++j)
                if (g + 4 * j < h2) tl[j] = col[(K3_STEP + g + 4 * j) * 64];
            __syncthreads();
#pragma unroll
            for (int j = 0; j < TJ; ++j)
                if (g + 4 * j < h2) col[(g + 4 * j) * 64] = tl[j];
        }
    }
}

// Rungs of the runtime-radius kernels: the template instance each getter (kt_*_legacy.hip)
// picks for a radius.  The getters and of3d_plan_geometry's "runtime_radius" both call these,
// so the report cannot drift from the launch.
// k_prod_wy<F, NP, TJ>: <= 24 for rw <= 48
constexpr int k3_tj(int rw) {
    const int tj = (2 * rw + 3) / 4;
    return tj <= 8 ? 8 : (tj <= 12 ? 12 : 24);
}

// ---------------------------------------------------------------------------
// K4: W x pass over NF fields.  Block = 64 rows x K4_TX x-outputs of one
// plane; lane = row, so each thread walks its row with a register-rotated
// window (K4_R outputs) over an LDS tile of odd pitch (conflict-free column
// access); results go back through LDS for coalesced row stores.
// ---------------------------------------------------------------------------
constexpr int K4_R = 8, K4_TX = 4 * K4_R, K4_ROWS = 64;

// Streaming form: a block owns 64 rows of one plane and one field, and marches
// along x K4_TX columns at a time.  The LDS window holds columns
// x' = x0 .. x0 + K4_TX + 2ha - 1 (x' = x + ha) of every row, ha = rw rounded
// up to 16 columns, so every 32-column fetch starts on a 128-byte line (odd
// pitch so lane = row reads are conflict-free); after each step the last 2ha
// columns move to the front.  Results leave through a transposing LDS tile for
// coalesced row stores; the next step's columns are fetched into registers
// during the current pass.
constexpr int k4_halo(int rw) { return (rw + 15) & ~15; }

template <typename F, int NF, int TJ>  // TJ >= ceil(2ha / 32): tail column groups per loader lane
__global__ __launch_bounds__(256, TJ == 1 ? 3 : 2) void k_wx(const F* __restrict__ P, F* __restrict__ Q, int ny,
                                                             int nx, size_t fs, const F* __restrict__ hw,
                                                             const F* __restrict__ hwr, int rw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* sm = reinterpret_cast<F*>(smem_raw);
    const int ha = k4_halo(rw);
    const int h2 = 2 * ha;
    const int PP = (K4_TX + h2) | 1;
    constexpr int OP = K4_TX + 1;
    F* so = sm + K4_ROWS * PP;  // output tile [row][K4_TX]
    const int lane = threadIdx.x, g = threadIdx.y;
    const int y0 = blockIdx.y * K4_ROWS;
    const int f = blockIdx.z % NF;
    const size_t pl = (size_t)(blockIdx.z / NF) * ny * nx;
    const F* src = P + f * fs + pl;
    F* dst = Q + f * fs + pl;
    // loader mapping: lanes 0..31 / 32..63 -> two rows, 32 consecutive columns
    const int lc = lane & 31, lr = (lane >> 5) + 2 * g;  // rows lr, lr + 8, ..., lr + 56
    int roff[8];  // row offsets (ny * nx < 2^31 per plan)
#pragma unroll
    for (int j = 0; j < 8; ++j) roff[j] = min(y0 + lr + 8 * j, ny - 1) * nx;
    auto colv = [&](int j, int xp) { return src[roff[j] + clampi(xp - ha, 0, nx - 1)]; };
    for (int xp = lc; xp < h2; xp += 32)
#pragma unroll
        for (int j = 0; j < 8; ++j) sm[(lr + 8 * j) * PP + xp] = colv(j, xp);
    F rv[8];
    auto fetch = [&](int xp0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) rv[j] = colv(j, xp0 + lc);
    };
    fetch(h2);
    F tl[TJ][8];
    for (int x0 = 0; x0 < nx; x0 += K4_TX) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sm[(lr + 8 * j) * PP + h2 + lc] = rv[j];
        __syncthreads();
        const bool more = x0 + K4_TX < nx;
        if (more) fetch(x0 + K4_TX + h2);
        F out[K4_R];
        lds_pass<K4_R, false, (TJ > 1)>(sm + lane * PP, 1, ha + g * K4_R, hw, hwr, rw, out);
#pragma unroll
        for (int i = 0; i < K4_R; ++i) so[lane * OP + g * K4_R + i] = out[i];
        if (more) {
#pragma unroll
            for (int t = 0; t < TJ; ++t)
                if (lc + 32 * t < h2)
#pragma unroll
                    for (int j = 0; j < 8; ++j) tl[t][j] = sm[(lr + 8 * j) * PP + K4_TX + lc + 32 * t];
        }
        __syncthreads();
        const int x = x0 + lc;
        if (x < nx)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int y = y0 + lr + 8 * j;
                if (y < ny) dst[(size_t)y * nx + x] = so[(lr + 8 * j) * OP + lc];
            }
        if (more) {
#pragma unroll
            for (int t = 0; t < TJ; ++t)
                if (lc + 32 * t < h2)
#pragma unroll
                    for (int j = 0; j < 8; ++j) sm[(lr + 8 * j) * PP + lc + 32 * t] = tl[t][j];
        }
    }
}

// k_wx<F, NF, TJ>: <= 3 for rw <= 48
constexpr int k4_tj(int rw) {
    const int tj = (2 * k4_halo(rw) + 31) / 32;
    return tj <= 1 ? 1 : (tj == 2 ? 2 : 3);
}

// ---------------------------------------------------------------------------
// K34: products + W y + W x in one pass (calc_flow.py:300-313 y and x passes;
// 2D :133-141), so the W-y result never goes to HBM.
//
// Block = one product of one plane, a column block of CW = blockDim.x staged
// columns (TX outputs + RW halo columns each side, clamped at the volume
// edge), one chunk of rows.  Thread = staged column, marching down its rows:
//   phase A (W y, registers only): the column's products live in a register
//     ring of NR slots (row j in slot (j - y0 + RW) mod NR); the loop is
//     unrolled by NR so every slot index is a compile-time constant, no moves,
//     no LDS reads.  Gradient loads run PD rows ahead (raw ring of PD).  Each
//     step writes its W-y row value into an LDS tile row (S rows per tile).
//   phase B (W x, every S rows): the tile's S rows x TX columns through
//     lds_pass (RB = 4 consecutive columns per item, lane = tile row, odd pitch),
//     results through an LDS out tile to coalesced row stores.
// Blocks are numbered XCD-aware: the blocks of one (plane, row chunk) group
// share blockIdx.x % 8 (one XCD's L2 under round-robin placement), so the four
// gradient rows that 9 products x column blocks read come from one L2.
// ---------------------------------------------------------------------------
constexpr int k34_nr(int rw, int s) { return ((2 * rw + 2 + s - 1) / s) * s; }
// K34 block -> (plane zl, row chunk yc, column block bx, product p).  The linear workgroup id
// b runs on XCD b % 8 (round-robin dispatch), so blocks that should share an L2 share b % 8:
// group g = (plane, run of cpg row chunks) = (b / 8 / mb) * 8 + b % 8, members (chunk in the
// run, product, column block).  (A chunk-major order — each XCD running its planes' row chunks
// one after another — measured slower everywhere, round 4: profiles/r04/ab_k34_cm.txt.)
struct K34Blk {
    int zl, yc, bx, p;
    bool ok;
};
template <int NP>
__device__ __forceinline__ K34Blk k34_block(int nbx, int nyb, int cpg, int ngroups) {
    const int kb = blockIdx.x >> 3, xcd = blockIdx.x & 7;
    K34Blk r;
    const int mb = cpg * NP * nbx;
    const int g = (kb / mb) * 8 + xcd;
    int m = kb % mb;
    r.bx = m % nbx;
    m /= nbx;
    r.p = m % NP;
    const int ycl = m / NP, nyg = (nyb + cpg - 1) / cpg;
    r.zl = g / nyg;
    r.yc = (g % nyg) * cpg + ycl;
    r.ok = g < ngroups && r.yc < nyb;
    return r;
}

// dynamic LDS of a K34 block: two W-y tiles of s rows at pitch cwp, es bytes an element; packed:
// k_prod_wyx_pk's two tiles of s / 2 row pairs of float2 at pitch cwp, no row offsets
constexpr size_t k34_lds(int s, int cwp, size_t es, bool packed = false) {
    return packed ? (size_t)s * cwp * 8 : (size_t)2 * k34_tile(s, cwp) * es;
}

// W-xy hand-off layout (K34 writes, K5c reads; csrc/of3d_host.hip picks it per plan).
// zt == 0: field-major planes [z][y][x].  zt > 0 (zt = the workspace's planes): z-tiled
// [y][x / 32][z][32] — K5c's block (32 columns of one row, ZC + 2 RW planes) then reads each field
// window as ONE contiguous run instead of ZC + 2 RW pieces of 256 B a plane apart: the window
// reads alone take 0.385 instead of 0.488 ms at c3, 3.13 instead of 4.0-4.2 ms at c4
// (tools/mb_window.hip).  K34 stores per tile of rows from yb: a buffer descriptor at the tile's
// first row and 32-bit per-lane byte offsets (a tile of S rows spans S nx zt elements), through one
// branch-free formula whose uniform parameters select the layout (a per-store select of the two
// formulas cost the lockstep K34 36 VGPRs: 3 -> 2 waves per SIMD at c2).
struct WxyMap {
    unsigned rs, cm, msk, sh;  // row stride (bytes); column-tile multiplier, mask, shift
};
template <typename F>
__device__ __forceinline__ WxyMap wxy_map(int nx, int zt) {
    constexpr unsigned ES = sizeof(F);
    return zt ? WxyMap{(unsigned)nx * (unsigned)zt * ES, (unsigned)zt * 32u, 31u, 5u}
              : WxyMap{(unsigned)nx * ES, 0u, ~0u, 31u};
}
template <typename F>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wxy_rsrc(F* Qp, int zl, int yb, int ny, int nx, int zt) {
    return zt ? buf_rsrc(Qp + ((size_t)yb * nx * zt + (size_t)zl * 32)) : buf_rsrc(Qp + ((size_t)zl * ny + yb) * nx);
}
// byte offset of row r (of the tile) at column x (x .. x + RB - 1 in one 32-column tile: RB | 32 and
// x a multiple of RB); plain planes: r nx + x (x >> 31 = 0, mask all ones)
template <typename F>
__device__ __forceinline__ unsigned wxy_off(const WxyMap& m, int r, int x) {
    const unsigned ux = (unsigned)x;
    return (unsigned)r * m.rs + ((ux >> m.sh) * m.cm + (ux & m.msk)) * (unsigned)sizeof(F);
}

// ---- the parts the three K34 kernels share (k_prod_wyx, k_prod_wyx_ws, k_prod_wyx_pk) ----
// Force-inlined into the same arithmetic order in each kernel.  A kernel uses a part unless the
// part moves the registers, scratch or occupancy of one of its instances, or measurably slows it
// (which kernel uses which part; the ring prologue, the march loop and the tail
// store stay written out in each kernel).

// Block geometry: output rows [y0, y0 + nrows) of [yb0, yb1) (row-slab plans: the rank's own
// rows; loads still clamp at [0, ny)), outputs [xo0, xo0 + txu) of the row, and the staged
// columns, tile position i <-> column xo0 - RW + i.
// UQ = false (duplicate staging): thread t stages column clamp(xo0 - RW + t) at position t, halo
//   positions outside the volume (mode='nearest') recomputed as duplicates of the edge column
//   (txu + 2 RW <= blockDim.x by the host's geometry); no pads.
// UQ = true (unique staging): the block's outputs and their W-x halo inside the volume, each once
//   ([sxs, sxs + ns), ns <= the block's staging threads by the host's geometry): thread t holds
//   column sxs + t at position padL + t (the packed kernel: a column pair per thread); the padL / padR
//   positions outside the volume are edge replicas copied once per tile (no halo work at all
//   for a block covering the whole row).
struct K34Geo {
    int zl, yc, bx, p;
    int y0, nrows, xo0, txu, sxs, ns, padL, padR;
};
template <bool UQ>
__device__ __forceinline__ K34Geo k34_geo(const K34Blk& b, int tx, int nyc, int yb0, int yb1, int nx, int rw) {
    K34Geo g;
    g.zl = b.zl, g.yc = b.yc, g.bx = b.bx, g.p = b.p;
    g.y0 = yb0 + b.yc * nyc;
    g.nrows = min(nyc, yb1 - g.y0);
    g.xo0 = b.bx * tx;
    g.txu = min(tx, nx - g.xo0);  // useful outputs of this block
    g.sxs = UQ ? max(g.xo0 - rw, 0) : g.xo0 - rw;
    g.ns = UQ ? min(g.xo0 + g.txu + rw, nx) - g.sxs : g.txu + 2 * rw;
    g.padL = UQ ? g.sxs - (g.xo0 - rw) : 0;
    g.padR = UQ ? (g.xo0 + g.txu + rw) - (g.sxs + g.ns) : 0;
    return g;
}

// Product sources: the two gradient fields of product p of NP (nibble tables as k_prod_wy), in
// the plane at element offset pl, as buffer descriptors
struct K34Src {
    __amdgpu_buffer_rsrc_t a, b;
};
template <int NP, typename F>
__device__ __forceinline__ K34Src k34_src(const F* G, size_t fs, size_t pl, int p) {
    constexpr unsigned long long pa = NP == 9 ? 0x311222312ull : 0x12212ull;
    constexpr unsigned long long pb = NP == 9 ? 0x313231000ull : 0x12100ull;
    const auto a = buf_rsrc(G + (size_t)((pa >> (4 * p)) & 15u) * fs + pl);
    const auto b = buf_rsrc(G + (size_t)((pb >> (4 * p)) & 15u) * fs + pl);
    return {a, b};
}
// byte offset of ring row idx of a block (row y0 - RW + idx, clamped to the plane; rowb bytes per row)
template <int RW>
struct K34Rows {
    int y0, ny;
    unsigned rowb;
    __device__ __forceinline__ unsigned off(int idx) const { return (unsigned)clampi(y0 - RW + idx, 0, ny - 1) * rowb; }
};

// Edge replicas of a unique-staging tile, copied once per tile by the wave that wrote the edge
// column (its own LDS writes are ordered before its reads).  The wave index sits in an SGPR: the
// branches on lpad / rpad (this wave holds column 0 in lane 0 / holds column nx - 1) are scalar, not
// exec-masked; ln: the lane.
// ROWS tile rows of V, row r at tile + row_at(r)
template <int ROWS, typename V, typename RowAt>
__device__ __forceinline__ void k34_replicas(V* tile, RowAt row_at, bool lpad, bool rpad, int ln, const K34Geo& g) {
    if (lpad) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            V* row = tile + row_at(r);
            const V v = row[g.padL];
            if (ln < g.padL) row[ln] = v;
        }
    }
    if (rpad) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            V* row = tile + row_at(r);
            const V v = row[g.padL + g.ns - 1];
            if (ln < g.padR) row[g.padL + g.ns + ln] = v;
        }
    }
}

// Phase A of one thread: the register ring of NR product rows (row j in slot (j - y0 + RW) mod NR)
// and the raw gradient rows PD ahead (ra, rb); ld(descriptor, row offset): this thread's staged
// column of one gradient row.  The prologue in the kernels fills slots 0 .. 2 RW and the first
// PD prefetch rows.
// Step j of the ring period starting at row u0: the W-y values a0, a1 of rows j, j + 1.  Two
// rows per step, their tap chains interleaved (ILP: a single chain issues one fp64 op per
// dependent latency).  Row j + 1's new product lands in row j's outermost slot, so it is
// written after row j's first tap.
// FENCED: the two chains side by side: without the two empty asm fences the scheduler issued
// half of a 16-wave producer's ops right behind the op they depend on; with them 2 % (c3 K34
// 1.665 -> 1.631 ms, c4 equal: profiles/r04/ab_k34ilp/).  Same ops, same order per chain
// (bit-identical).  The packed fp32 kernel spills with it and the lockstep one keeps its form.
template <int j, int RW, bool FENCED, typename V, int NR, int PD, typename Ld>
__device__ __forceinline__ void k34_ring_step(V (&ring)[NR], V (&ra)[PD], V (&rb)[PD], Ld ld, const K34Src& src,
                                              const K34Rows<RW>& rows, int u0, const V (&h)[RW + 1], V& a0, V& a1) {
    static_assert(NR % PD == 0, "ring sizes");
    constexpr int ic = j + 2 * RW + 1, ic1 = ic + 1;
    ring[ic % NR] = ra[ic % PD] * rb[ic % PD];
    const unsigned o = rows.off(u0 + ic + PD);
    ra[ic % PD] = ld(src.a, o);
    rb[ic % PD] = ld(src.b, o);
    V p1 = ra[ic1 % PD] * rb[ic1 % PD];
    const unsigned o1 = rows.off(u0 + ic1 + PD);
    ra[ic1 % PD] = ld(src.a, o1);
    rb[ic1 % PD] = ld(src.b, o1);
    a0 = ring[(j + RW) % NR] * h[0];
    a1 = ring[(j + 1 + RW) % NR] * h[0];
    a0 = a0 + (ring[j % NR] + ring[(j + 2 * RW) % NR]) * h[RW];
    a1 = a1 + (ring[(j + 1) % NR] + ring[(j + 1 + 2 * RW) % NR]) * h[RW];
    ring[ic1 % NR] = p1;  // slot of row j - RW (NR = 2 RW + 2): free now
#pragma unroll
    for (int k = RW - 1; k >= 1; --k) {
        if constexpr (FENCED) {
            V s0 = ring[(j + RW - k) % NR] + ring[(j + RW + k) % NR];
            V s1 = ring[(j + 1 + RW - k) % NR] + ring[(j + 1 + RW + k) % NR];
            asm volatile("" : "+v"(s0), "+v"(s1));
            s0 = s0 * h[k];
            s1 = s1 * h[k];
            asm volatile("" : "+v"(s0), "+v"(s1));
            a0 = a0 + s0;
            a1 = a1 + s1;
        } else {
            a0 = a0 + (ring[(j + RW - k) % NR] + ring[(j + RW + k) % NR]) * h[k];
            a1 = a1 + (ring[(j + 1 + RW - k) % NR] + ring[(j + 1 + RW + k) % NR]) * h[k];
        }
    }
}

// Phase-B items of a tile of S rows (RB consecutive outputs each).  Item -> lane, conflict-free
// for both LDS read forms (ds_read_b64: 32-lane groups, 64 banks; ds_read2_b64: 16-lane groups,
// 32 banks): lane bits b5..b0 give row (b3b2) + 4 b5 and segment (b1b0) + 4 b4, and row r starts
// at k34_row(r) = r mod 4 (mod 32 doubles), so a lane reads at (b3b2) + 4 (b1b0) + 16 b4 (mod 32):
// 16 distinct mod 16, 32 distinct mod 32.  S = 4: rows (b3b2), segment (b1b0) + 4 b4 + 8 b5.
template <int S>
struct K34Items {
    static constexpr int RPW = S < 8 ? S : 8, SPW = 64 / RPW;  // rows / segments per wave-item group
    static constexpr int RG = S / RPW;                          // row groups
    static __device__ __forceinline__ void at(int i, int& r, int& sg) {
        const int l = i & 63, wg = i >> 6;
        r = (wg % RG) * RPW + ((l >> 2) & 3) + (S >= 8 ? 4 * (l >> 5) : 0);
        sg = (wg / RG) * SPW + (l & 3) + 4 * ((l >> 4) & 1) + (S >= 8 ? 0 : 8 * (l >> 5));
    }
};

// The lockstep K34: every wave runs phase A, then phase B of the same tile.
// OCC: waves per SIMD the register budget is cut for (3: 168 VGPRs; 2: 256, for 8-wave blocks,
// which run one per CU anyway); PDX: gradient prefetch rows (0: as far as OCC 3 allows);
// DB: LDS prefetch distance of the phase-B pass; UQ: staging (K34Geo).
// RB: W-x outputs per phase-B item (RB 2 measured slower: c2 +16 %, c3 +15 %; not instantiated)
template <typename F, int NP, int RW, int S, int RB = 4, int OCC = 3, int PDX = 0, int DB = 2,
          bool UQ = false>
__global__ __launch_bounds__(512, OCC) void k_prod_wyx(const F* __restrict__ G, F* __restrict__ Q, int ny,
                                                       int nx, size_t fs, const F* __restrict__ hw, int tx,
                                                       int nyc, int nbx, int nyb, int cpg, int ngroups, int yb0,
                                                       int yb1, int zt) {
    // gradient prefetch distance (rows): as far as 168 VGPRs (3 waves/SIMD) allow
    constexpr int NR = k34_nr(RW, S), PD = PDX ? PDX : (sizeof(F) == 8 ? (RW >= 18 ? 2 : 4) : (RW >= 18 ? 4 : 8));
    static_assert(NR % S == 0, "ring sizes");
    using It = K34Items<S>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* sw = reinterpret_cast<F*>(smem_raw);  // two W-y tiles [2][S][cwp] (tile n in buffer n & 1)
    const int cwp = UQ ? k34_pitch(min(tx, nx), RW) : (int)blockDim.x + 1;
    const int t = threadIdx.x;
    // XCD-aware block decode: group g = (plane, run of cpg row chunks), member m = (chunk in the
    // run, product, column block): one group's blocks share an XCD and are dispatched together
    const K34Blk kbk = k34_block<NP>(nbx, nyb, cpg, ngroups);
    if (!kbk.ok) return;
    const K34Geo g = k34_geo<UQ>(kbk, tx, nyc, yb0, yb1, nx, RW);
    // waves with no staged column leave at once; barriers count only the waves still running
    const int wa = (g.ns + 63) >> 6, ca = 64 * wa;
    if (t >= ca) return;
    const unsigned vof = (unsigned)clampi(g.sxs + t, 0, nx - 1) * (unsigned)sizeof(F);  // staged column of this thread
    // wave index in an SGPR: the edge-replica branches are scalar, not exec-masked
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6), ln = t & 63;
    const bool lpad = UQ && g.padL > 0 && wv == 0;                  // wave 0 holds column 0 in lane 0
    const bool rpad = UQ && g.padR > 0 && wv == ((g.ns - 1) >> 6);  // this wave holds column nx - 1
    // UQ: lanes past ns (last wave) compute a duplicate and store it past the row's positions
    // (pitch cwp >= txu + 2 RW + 1; that slot only feeds outputs >= txu, never stored)
    const int wpos = !UQ ? t : (t < g.ns ? g.padL + t : g.padL + g.ns + g.padR);
    const K34Src src = k34_src<NP>(G, fs, (size_t)g.zl * ny * nx, g.p);
    F* const Qp = Q + (size_t)g.p * fs;
    const WxyMap wm = wxy_map<F>(nx, zt);
    const K34Rows<RW> rows{g.y0, ny, (unsigned)nx * (unsigned)sizeof(F)};
    F h[RW + 1];
#pragma unroll
    for (int k = 0; k <= RW; ++k) h[k] = hw[k];
    auto ld = [&](const __amdgpu_buffer_rsrc_t& r, unsigned o) { return buf_ld<F>(r, vof, o); };
    F ring[NR], ra[PD], rb[PD];
#pragma unroll
    for (int i = 0; i <= 2 * RW; ++i) {  // ring prologue (see k34_ring_step): products of rows 0 .. 2 RW
        const unsigned o = rows.off(i);
        ring[i] = ld(src.a, o) * ld(src.b, o);
    }
#pragma unroll
    for (int i = 0; i < PD; ++i) {  // and the first PD prefetch rows
        const unsigned o = rows.off(2 * RW + 1 + i);
        ra[(2 * RW + 1 + i) % PD] = ld(src.a, o);
        rb[(2 * RW + 1 + i) % PD] = ld(src.b, o);
    }
    const int nseg = (g.txu + RB - 1) / RB;
    const int nsgw = (nseg + It::SPW - 1) / It::SPW;
    // phase B: W x over tile buffer `tile` (rows r < S), rows [yb, yb + nr) stored.  One barrier
    // per tile: the other buffer is being filled by phase A meanwhile.
    auto phase_b = [&](const F* tile, int yb, int nr) {
        lds_barrier();
        const auto rq_ = wxy_rsrc(Qp, g.zl, yb, ny, nx, zt);
        for (int i = t; i < 64 * It::RG * nsgw; i += ca) {
            int r, sg;
            It::at(i, r, sg);
            if (sg >= nseg) continue;
            F out[RB];
            lds_pass_c<RB, RW, DB>(tile + k34_row(r, cwp), 1, RW + RB * sg, h, out);
            if (r < nr) {
                // row offset per lane in voffset (a divergent soffset would be a waterfall loop)
                const int c0 = RB * sg;
                const unsigned vo = wxy_off<F>(wm, r, g.xo0 + c0);
                if (c0 + RB <= g.txu) {
                    buf_st_n<F, RB>(out, rq_, vo, 0);
                } else {
                    for (int e = 0; e < RB; ++e)
                        if (c0 + e < g.txu) buf_st<F>(out[e], rq_, vo + e * (unsigned)sizeof(F), 0);
                }
            }
        }
    };
    // the march: ring periods of NR rows unrolled (every ring slot index a compile-time constant),
    // tiles of S rows alternating between the two buffers
    for (int u0 = 0; u0 < g.nrows; u0 += NR) {
        bool done = false;
        [&]<int... H>(std::integer_sequence<int, H...>) {
            (
                [&] {
                    if (done) return;
                    constexpr int h0 = H * S;
                    F* tile = sw + (((u0 + h0) / S) & 1) * k34_tile(S, cwp);
                    [&]<int... J>(std::integer_sequence<int, J...>) {
                        (
                            [&] {
                                constexpr int j = h0 + 2 * J;  // step within the ring period
                                F a0, a1;
                                k34_ring_step<j, RW, false>(ring, ra, rb, ld, src, rows, u0, h, a0, a1);
                                (tile + k34_row(j % S, cwp))[wpos] = a0;
                                (tile + k34_row((j + 1) % S, cwp))[wpos] = a1;
                            }(),
                            ...);
                    }(std::make_integer_sequence<int, S / 2>{});
                    const int yb = u0 + h0;
                    if constexpr (UQ) k34_replicas<S>(tile, [&](int r) { return k34_row(r, cwp); }, lpad, rpad, ln, g);
                    phase_b(tile, g.y0 + yb, min(S, g.nrows - yb));
                    if (yb + S >= g.nrows) done = true;
                }(),
                ...);
        }(std::make_integer_sequence<int, NR / S>{});
        if (done) break;
    }
}

// K34 with specialised waves (unique staging, 1024 threads): waves 0..7 are producers —
// phase A (products + W y, one staged column per thread, register ring) writing the W-y
// tile — and waves 8..15 consumers — phase B (W x + stores) of the PREVIOUS tile, so the
// producers' gradient loads and the consumers' LDS reads / stores overlap each other's
// arithmetic instead of alternating in lockstep.  One barrier per tile, two tile buffers:
// producers write tile t + 1 while consumers read tile t.  Phase-A step, edge replicas and item
// decode are the parts k_prod_wyx uses (same arithmetic and order: bit-identical); the ring
// prologue, the march loop and the tail store are this kernel's own copies.  128-VGPR budget (16 waves per CU): prefetch depth PD.
// Ablation at c3 (round 2, timing-only experiment builds since removed): without the W-xy
// stores 1.13 ms vs 1.72 — but that build had no phase-B arithmetic either (dead code without
// its stores; checked in the device assembly in round 3), i.e. the producers alone; gradient
// loads from one cache-resident row 1.48.  Staging the stores through a wave-private LDS transpose (whole
// rows per store instruction) measured slower (1.88 ms): the 72 B/voxel W-xy hand-off to
// K5c itself, not its access pattern, is the cost.
// (12-wave blocks — 4 consumer waves, 168 VGPRs, deeper prefetch, 8-row tiles — measured
// slower: c3 1.95 vs 1.72 ms, c2 0.27 vs 0.19: the 16-wave occupancy hides more.)
// The producers run the fenced phase-A step (k34_ring_step).
// NPW: producer waves (staged columns 64 NPW), the other 16 - NPW consume.  8 + 8 suits a row
// whose blocks stage 512 columns (c3: the whole 512-wide row, no halo); 9 + 7 lets a 1024-wide
// row (c4) take two blocks of 512 outputs + 15 halo columns (527 staged) instead of three of 344
// (374 staged: two of the eight producer waves idle, a third of the consumers' capacity unused).
template <typename F, int NP, int RW, int S, int PD = 2, int DB = 2, int NPW = 8>
__global__ __launch_bounds__(1024) void k_prod_wyx_ws(const F* __restrict__ G, F* __restrict__ Q, int ny, int nx,
                                                      size_t fs, const F* __restrict__ hw, int tx, int nyc, int nbx,
                                                      int nyb, int cpg, int ngroups, int yb0, int yb1, int zt) {
    constexpr int RB = 4, CWA = 64 * NPW, NCT = 1024 - CWA;  // producer threads; consumer threads
    constexpr int NR = k34_nr(RW, S);
    static_assert(NR % S == 0, "ring sizes");
    using It = K34Items<S>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* sw = reinterpret_cast<F*>(smem_raw);  // two W-y tiles [2][S][cwp]
    const int cwp = k34_pitch(min(tx, nx), RW);
    const int t = threadIdx.x;
    const K34Blk kbk = k34_block<NP>(nbx, nyb, cpg, ngroups);
    if (!kbk.ok) return;
    const K34Geo g = k34_geo<true>(kbk, tx, nyc, yb0, yb1, nx, RW);
    const int wa = (g.ns + 63) >> 6;
    const bool prod = t < CWA;
    // producer waves with no staged column: every wave still takes one barrier per tile
    // (a wave-uniform test, so the whole wave takes this branch)
    if (prod && __builtin_amdgcn_readfirstlane(t >> 6) >= wa) {
        for (int tt = 0; tt < (g.nrows + S - 1) / S; ++tt) lds_barrier();
        return;
    }
    F h[RW + 1];
#pragma unroll
    for (int k = 0; k <= RW; ++k) h[k] = hw[k];
    const size_t pl = (size_t)g.zl * ny * nx;
    const K34Rows<RW> rows{g.y0, ny, (unsigned)nx * (unsigned)sizeof(F)};
    const int ntiles = (g.nrows + S - 1) / S;
    if (prod) {
        const unsigned vof = (unsigned)clampi(g.sxs + t, 0, nx - 1) * (unsigned)sizeof(F);
        const int wv = __builtin_amdgcn_readfirstlane(t >> 6), ln = t & 63;
        const bool lpad = g.padL > 0 && wv == 0;
        const bool rpad = g.padR > 0 && wv == ((g.ns - 1) >> 6);
        const int wpos = t < g.ns ? g.padL + t : g.padL + g.ns + g.padR;
        const K34Src src = k34_src<NP>(G, fs, pl, g.p);
        auto ld = [&](const __amdgpu_buffer_rsrc_t& r, unsigned o) { return buf_ld<F>(r, vof, o); };
        F ring[NR], ra[PD], rb[PD];
#pragma unroll
        for (int i = 0; i <= 2 * RW; ++i) {  // ring prologue and march as in k_prod_wyx
            const unsigned o = rows.off(i);
            ring[i] = ld(src.a, o) * ld(src.b, o);
        }
#pragma unroll
        for (int i = 0; i < PD; ++i) {
            const unsigned o = rows.off(2 * RW + 1 + i);
            ra[(2 * RW + 1 + i) % PD] = ld(src.a, o);
            rb[(2 * RW + 1 + i) % PD] = ld(src.b, o);
        }
        for (int u0 = 0; u0 < g.nrows; u0 += NR) {
            bool done = false;
            [&]<int... H>(std::integer_sequence<int, H...>) {
                (
                    [&] {
                        if (done) return;
                        constexpr int h0 = H * S;
                        F* tile = sw + (((u0 + h0) / S) & 1) * k34_tile(S, cwp);
                        [&]<int... J>(std::integer_sequence<int, J...>) {
                            (
                                [&] {
                                    constexpr int j = h0 + 2 * J;
                                    F a0, a1;
                                    k34_ring_step<j, RW, true>(ring, ra, rb, ld, src, rows, u0, h, a0, a1);
                                    tile[k34_row(j % S, cwp) + wpos] = a0;
                                    tile[k34_row((j + 1) % S, cwp) + wpos] = a1;
                                }(),
                                ...);
                        }(std::make_integer_sequence<int, S / 2>{});
                        k34_replicas<S>(tile, [&](int r) { return k34_row(r, cwp); }, lpad, rpad, ln, g);
                        lds_barrier();  // tile published; the consumers are done with the other buffer
                        if (u0 + h0 + S >= g.nrows) done = true;
                    }(),
                    ...);
            }(std::make_integer_sequence<int, NR / S>{});
            if (done) break;
        }
    } else {
        const int tb = t - CWA;
        F* const Qp = Q + (size_t)g.p * fs;
        const WxyMap wm = wxy_map<F>(nx, zt);
        const int nseg = (g.txu + RB - 1) / RB;
        const int nsgw = (nseg + It::SPW - 1) / It::SPW;
        // 7 consumer waves (9 producers): a tile whose item groups are one more than whole rounds
        // of 7 (a 512-wide row at 4 or 8 rows: 8 groups) would make ONE wave run that group as a
        // second round (its SIMD then carries ~17 % more VALU work per tile than the others); that
        // group's 256 outputs go instead as single outputs to the first 4 consumer waves, one per
        // lane, which spreads them over 4 SIMDs (same arithmetic per output: bit-identical)
        constexpr int NCW = NCT / 64, COLS = It::SPW * RB;
        constexpr bool SOLO = k34_solo && sizeof(F) == 8;
        const int ngrp = It::RG * nsgw;
        const bool spread = NPW != 8 && It::RG == 1 && ngrp % NCW == 1;
        const int nmain = spread ? ngrp - 1 : ngrp;
        for (int tt = 0; tt < ntiles; ++tt) {
            lds_barrier();  // tile tt written
            const F* tile = sw + (tt & 1) * k34_tile(S, cwp);
            const int yb = g.y0 + tt * S, nr = min(S, g.nrows - tt * S);
            const auto rq_ = wxy_rsrc(Qp, g.zl, yb, ny, nx, zt);
            if (spread && tb < It::RPW * COLS) {  // the leftover group: row tb / COLS, one column per lane
                const int r = tb / COLS, c0 = (ngrp - 1) * COLS + tb % COLS;
                if (c0 < g.txu) {
                    F o1[1];
                    lds_pass_c<1, RW, DB, false, SOLO>(tile + k34_row(r, cwp), 1, RW + c0, h, o1);
                    if (r < nr) buf_st<F>(o1[0], rq_, wxy_off<F>(wm, r, g.xo0 + c0), 0);
                }
            }
            for (int i = tb; i < 64 * nmain; i += NCT) {
                int r, sg;
                It::at(i, r, sg);
                if (sg >= nseg) continue;
                F out[RB];
                lds_pass_c<RB, RW, DB, false, SOLO>(tile + k34_row(r, cwp), 1, RW + RB * sg, h, out);
                if (r < nr) {
                    const int c0 = RB * sg;
                    const unsigned vo = wxy_off<F>(wm, r, g.xo0 + c0);
                    if (c0 + RB <= g.txu) {
                        buf_st_n<F, RB>(out, rq_, vo, 0);
                    } else {
                        for (int e = 0; e < RB; ++e)
                            if (c0 + e < g.txu) buf_st<F>(out[e], rq_, vo + e * (unsigned)sizeof(F), 0);
                    }
                }
            }
        }
    }
}

// Packed-fp32 K34 (OF3D_FP32 plans): k_prod_wyx_ws's producer / consumer split on CDNA's
// packed fp32 math (v_pk_mul_f32 / v_pk_add_f32: two lanes of work per instruction, each
// element rounded as the scalar op — bit-identical to the fp32 kernels).  8-wave blocks
// (two per CU): waves 0..3 producers, one PAIR of staged columns per thread (512 staged
// columns), phase A on float2 {column c, c + 1}; waves 4..7 consumers, phase B on float2
// {row 2p, row 2p + 1}.  The W-y tile is stored row-pair interleaved — tile2[p][x] =
// {W-y(2p, x), W-y(2p + 1, x)} — so both phases read and write aligned float2: the
// producer's two rows j, j + 1 of columns c, c + 1 are the pair row j / 2 at x = c, c + 1.
// Pair pitch P2 = 1 (mod 32) float2: the consumers' 4 pairs x 4 segments of a 16-lane
// group hit 32 distinct banks.  Ring, prefetch and tile double-buffering as k_prod_wyx_ws:
// k34_ring_step and k34_replicas on float2; the ring prologue, the march loop and the tail
// store are this kernel's own copies.
template <int NP, int RW, int S, int PD = 2, int DB = 2>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_prod_wyx_pk(const float* __restrict__ G, float* __restrict__ Q, int ny,
                                                     int nx, size_t fs, const float* __restrict__ hw, int tx,
                                                     int nyc, int nbx, int nyb, int cpg, int ngroups, int yb0,
                                                     int yb1, int zt) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    constexpr int RB = 4, NPT = 256;  // outputs per consumer item; producer (= consumer) threads
    constexpr int NR = k34_nr(RW, S);
    static_assert(NR % PD == 0 && NR % S == 0 && (S == 8 || S == 4), "ring sizes, whole row pairs");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    f2* sw = reinterpret_cast<f2*>(smem_raw);  // two tiles [2][S / 2][P2]
    const int P2 = k34_pitch(min(tx, nx), RW);
    const int TB = (S / 2) * P2;  // float2 per tile buffer
    const int t = threadIdx.x;
    const K34Blk kbk = k34_block<NP>(nbx, nyb, cpg, ngroups);
    if (!kbk.ok) return;
    const K34Geo g = k34_geo<true>(kbk, tx, nyc, yb0, yb1, nx, RW);
    const int npair = (g.ns + 1) >> 1;  // column pairs staged
    const int wa = (npair + 63) >> 6;
    const bool prod = t < NPT;
    // producer waves with no staged column pair: every wave still takes one barrier per tile
    // (a wave-uniform test, so the whole wave takes this branch)
    if (prod && __builtin_amdgcn_readfirstlane(t >> 6) >= wa) {
        for (int tt = 0; tt < (g.nrows + S - 1) / S; ++tt) lds_barrier();
        return;
    }
    f2 h[RW + 1];
#pragma unroll
    for (int k = 0; k <= RW; ++k) h[k] = (f2){hw[k], hw[k]};
    const size_t pl = (size_t)g.zl * ny * nx;
    const K34Rows<RW> rows{g.y0, ny, (unsigned)nx * 4u};
    const int ntiles = (g.nrows + S - 1) / S;
    if (prod) {
        const int wv = __builtin_amdgcn_readfirstlane(t >> 6), ln = t & 63;
        const bool lpad = g.padL > 0 && wv == 0;
        const bool rpad = g.padR > 0 && wv == ((npair - 1) >> 6);
        const int wpos = g.padL + 2 * t;  // tile column of this thread's first staged column
        const K34Src src = k34_src<NP>(G, fs, pl, g.p);
        // the column pair as ONE 8-byte load (dword-aligned buffer load): columns c, c + 1 when
        // both are inside the row, else the row's last two with the last one duplicated (the
        // clamped pair of the scalar form)
        const int cp = g.sxs + 2 * t;
        const bool dup = cp > nx - 2;
        const unsigned vp = (unsigned)(dup ? nx - 2 : cp) * 4u;
        auto ld2 = [&](const __amdgpu_buffer_rsrc_t& r, unsigned o) {
            f2 v = __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(r, vp, o, 0));
            if (dup) v.x = v.y;
            return v;
        };
        f2 ring[NR], ra[PD], rb[PD];
#pragma unroll
        for (int i = 0; i <= 2 * RW; ++i) {  // ring prologue and march as in k_prod_wyx
            const unsigned o = rows.off(i);
            ring[i] = ld2(src.a, o) * ld2(src.b, o);
        }
#pragma unroll
        for (int i = 0; i < PD; ++i) {
            const unsigned o = rows.off(2 * RW + 1 + i);
            ra[(2 * RW + 1 + i) % PD] = ld2(src.a, o);
            rb[(2 * RW + 1 + i) % PD] = ld2(src.b, o);
        }
        for (int u0 = 0; u0 < g.nrows; u0 += NR) {
            bool done = false;
            [&]<int... H>(std::integer_sequence<int, H...>) {
                (
                    [&] {
                        if (done) return;
                        constexpr int h0 = H * S;
                        f2* tile = sw + (((u0 + h0) / S) & 1) * TB;
                        [&]<int... J>(std::integer_sequence<int, J...>) {
                            (
                                [&] {
                                    constexpr int j = h0 + 2 * J;
                                    f2 a0, a1;
                                    k34_ring_step<j, RW, false>(ring, ra, rb, ld2, src, rows, u0, h, a0, a1);
                                    // rows j, j + 1 (pair (j % S) / 2) at columns wpos, wpos + 1
                                    // (threads past the staged pairs write nothing: wpos would
                                    // run into the next pair row)
                                    if (t < npair) {
                                        f2* q = tile + ((j % S) / 2) * P2 + wpos;
                                        q[0] = (f2){a0.x, a1.x};
                                        q[1] = (f2){a0.y, a1.y};
                                    }
                                }(),
                                ...);
                        }(std::make_integer_sequence<int, S / 2>{});
                        k34_replicas<S / 2>(tile, [&](int q) { return q * P2; }, lpad, rpad, ln, g);
                        lds_barrier();  // tile published; the consumers are done with the other buffer
                        if (u0 + h0 + S >= g.nrows) done = true;
                    }(),
                    ...);
            }(std::make_integer_sequence<int, NR / S>{});
            if (done) break;
        }
    } else {
        const int tb = t - NPT;
        float* const Qp = Q + (size_t)g.p * fs;
        const WxyMap wm = wxy_map<float>(nx, zt);
        const int nseg = (g.txu + RB - 1) / RB;
        constexpr int PP = S / 2, SPW = 64 / PP;  // pairs per tile; segments per wave item
        const int nsgw = (nseg + SPW - 1) / SPW;
        for (int tt = 0; tt < ntiles; ++tt) {
            lds_barrier();  // tile tt written
            const f2* tile = sw + (tt & 1) * TB;
            const int yb = g.y0 + tt * S, nr = min(S, g.nrows - tt * S);
            const auto rq_ = wxy_rsrc(Qp, g.zl, yb, ny, nx, zt);
            for (int i = tb; i < 64 * nsgw; i += NPT) {
                const int l = i & 63, wg = i >> 6;
                const int pr = l % PP, sg = wg * SPW + l / PP;
                if (sg >= nseg) continue;
                f2 out[RB];
                lds_pass_c<RB, RW, DB>(tile + pr * P2, 1, RW + RB * sg, h, out);
                const int c0 = RB * sg;
#pragma unroll
                for (int e2 = 0; e2 < 2; ++e2) {
                    const int r = 2 * pr + e2;
                    if (r < nr) {
                        float o[RB];
#pragma unroll
                        for (int e = 0; e < RB; ++e) o[e] = e2 ? out[e].y : out[e].x;
                        const unsigned vo = wxy_off<float>(wm, r, g.xo0 + c0);
                        if (c0 + RB <= g.txu) {
                            buf_st_n<float, RB>(o, rq_, vo, 0);
                        } else {
                            for (int e = 0; e < RB; ++e)
                                if (c0 + e < g.txu) buf_st<float>(o[e], rq_, vo + e * 4u, 0);
                        }
                    }
                }
            }
        }
    }
}

}  // namespace

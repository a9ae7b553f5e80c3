#pragma once
// of3d_k12.hpp — K12: the gradient y, x and z passes in one kernel (pipeline overview:
// of3d_common.hpp).
#include <type_traits>
#include <utility>

#include "of3d_common.hpp"

namespace {

// ---------------------------------------------------------------------------
// K12: the gradient y, x and z passes in one kernel (calc_flow.py:279-288) — the four
// pre-z fields never leave the CU (K1c + K2c write and re-read them through HBM).
// Block = TY = 4 rows x TX = CW - 2 RD output columns (CW = 64 NWX staged columns: NWX waves
// per row, 3 in fp64, 2 in fp32), marching a chunk of output planes.  Wave w: part h = w % NWX
// (staged column c = 64 h + lane), role / row r = w / NWX.  Per input plane (one step):
//   staging (LDS-DMA): the plane's TY + 2 RD rows of dt0 and of the centre frame I (the
//     block's staged columns, 16-byte granules) go straight into LDS, a chunk of K (3, 2 or 1
//     where LDS is short) planes at a time, two chunks ahead (2 K plane slots): one chunk's loads
//     stay in flight while the previous chunk computes; one vmcnt(0) per chunk;
//   y passes (LDS -> registers): role 0 A1 = y(G)[dt0], role 1 A2 = y(D)[I], role 2
//     A3 = y(S)[I] of the thread's staged column (clamped at the global edge), results
//     into LDS tiles (two buffers);
//   x passes (LDS): thread (row r, staged column c) forms B1 = x(G)[A1], B2 = x(S)[A2],
//     B3 = x(D)[A3], B4 = x(S)[A3] for output column c - RD (lanes past the block's
//     outputs compute clamped duplicates and store nothing);
//   z passes (registers): B1..B4 enter per-thread register rings (NR = 2 RD + 2 slots for
//     the radius-RD fields, NRS = RD + 1 for the smooth ones; compile-time slots: the plane
//     loop is unrolled by NR); dt = z(G)[B1] and dz = z(D)[B4] leave once plane q + RD is
//     in, dy = z(S)[B2] and dx = z(S)[B3] once plane q + RS is.
// One barrier per step; the y passes of step s + 1 run beside the x / z passes of step s
// (the A tiles alternate), so each wave has two independent streams of work per step.
// Same expression order as K1c + K2c (scipy's), staged rows/columns clamped at the global
// edge, planes clamped to [0, nzc): bit-identical.  Blocks are numbered XCD-aware (the
// tiles of one XCD form a band of rows, so the halo rows of neighbouring tiles share an L2).
// Needs nx * sizeof(F) and nx * sizeof(T) multiples of 16 bytes and 16-byte aligned planes.
// ---------------------------------------------------------------------------
constexpr int K12_TY = 4;  // rows per block
// staged columns per block row: 64 per wave, k12_nwx waves per row.  fp64: 3 waves (192
// staged columns, 180 outputs at rd 6): 12-wave blocks = 3 waves per SIMD instead of 2 (the
// kernel is bound by each wave's dependent chain, so a third wave per SIMD is what pays), at
// 168 VGPRs (one x window live at a time) and one plane per DMA chunk (LDS); and 5 % of the
// staged columns of a 512-wide plane wasted instead of 13 %.  Same box: c3 K12 0.617 -> 0.462
// ms, c4 4.09 -> 3.37 ms (profiles/r04/ab_k12n3/).  fp32 keeps 2 (two 8-wave blocks per CU).
template <typename F>
__host__ __device__ constexpr int k12_nwx() { return sizeof(F) == 8 ? 3 : 2; }
template <typename F>
__host__ __device__ constexpr int k12_cw() { return 64 * k12_nwx<F>(); }
template <typename F>
__host__ __device__ constexpr int k12_threads() { return k12_cw<F>() * K12_TY; }
// z passes one step late (k_grad_xyz_c) in the fp32 kernels: c5 K12 18.2-18.5 -> 17.4 ms; the
// fp64 kernel measured slower so (c3 0.602 -> 0.645 ms, same box, profiles/r03_ab/k12_defer/)
template <typename F>
constexpr bool k12_defer() { return sizeof(F) == 4; }
template <typename F, int RD>
__host__ __device__ constexpr int k12_tx() { return k12_cw<F>() - 2 * RD; }
// LDS bytes of one staged plane: NRW rows of dt0 (CW + EPL columns) and of I (CW + EPL_T)
template <typename T, typename F, int RD>
__host__ __device__ constexpr int k12_slot_granules() {
    return (K12_TY + 2 * RD) * ((k12_cw<F>() * (int)sizeof(F)) / 16 + 1 + (k12_cw<F>() * (int)sizeof(T)) / 16 + 1);
}
template <typename T, typename F, int RD>
__host__ __device__ constexpr int k12_slot_bytes() { return ((k12_slot_granules<T, F, RD>() + 63) / 64) * 1024; }
// A tiles: [2 buffers][3 fields][even / odd copy][TY][AP]; the odd copy is the row
// shifted by one element, so every x-pass window starts 16-byte aligned in one of the two
// (pairs read as ds_read_b128: 4 LDS cycles per 16 B; ds_read2_b64 costs 16).  Pitch
// CW + 4 (132 / 196): the odd copy sits 128 B (mod 256) from the even one (conflict-free
// b128 groups).
template <typename F>
__host__ __device__ constexpr int k12_ap() { return k12_cw<F>() + 4; }
// fp64 (round 6): ONE copy per A row; the x windows read single 8-byte elements (ds_read_b64:
// 2 LDS cycles per 512 B, the b128 rate; kept from pairing into ds_read2_b64 by empty fences) —
// half the y-pass LDS writes and half the A-tile bytes, which buys the third DMA slot below.
// fp32 keeps the odd-shifted copies (its 4-byte reads would run at half rate).
constexpr bool k12_odd_fp64 = false;
constexpr bool k12_ysolo = true;  // fp64 y-pass reads of dt0 as single ds_read_b64s
template <typename F>
__host__ __device__ constexpr bool k12_odd() { return sizeof(F) == 4 || k12_odd_fp64; }
template <typename F>
__host__ __device__ constexpr int k12_a_bytes() {
    return 2 * 3 * (k12_odd<F>() ? 2 : 1) * K12_TY * k12_ap<F>() * (int)sizeof(F);
}
// planes per DMA chunk: 2 where two chunks of slots + the A tiles fit 80 KiB and the
// kernel's registers allow 4 waves per SIMD (fp32 rd 3 / 6: two 8-wave blocks per CU),
// else 3 where they fit 160 KiB, else 2
template <typename T, typename F, int RD>
__host__ __device__ constexpr int k12_k() {
    if (sizeof(F) == 4 && RD <= 6 && 4 * k12_slot_bytes<T, F, RD>() + k12_a_bytes<F>() <= 80 * 1024)
        return 2;
    if (6 * k12_slot_bytes<T, F, RD>() + k12_a_bytes<F>() <= 160 * 1024) return 3;
    return 4 * k12_slot_bytes<T, F, RD>() + k12_a_bytes<F>() <= 160 * 1024 ? 2 : 1;
}
// chunks of DMA slots: DEEP instances 3 (each plane's loads get two steps to land) for one-plane
// chunks of the non-deferred (fp64) kernel where three slots fit beside the A tiles, else 2 (one
// step).  The host takes DEEP for marches of >= 128 planes: same box, c4 (256-plane marches) K12
// 3.19 -> 3.10 ms; c3 (64) equal; c2 (32) 0.088 -> 0.091 (profiles/r06/abk12/)
template <typename T, typename F, int RD, bool DEEP>
__host__ __device__ constexpr int k12_nch() {
    return DEEP && !k12_defer<F>() && k12_k<T, F, RD>() == 1 &&
                   3 * k12_slot_bytes<T, F, RD>() + k12_a_bytes<F>() <= 160 * 1024
               ? 3
               : 2;
}
template <typename T, typename F, int RD, bool DEEP = false>
__host__ __device__ constexpr int k12_lds_bytes() {
    return k12_nch<T, F, RD, DEEP>() * k12_k<T, F, RD>() * k12_slot_bytes<T, F, RD>() + k12_a_bytes<F>();
}

template <typename T, typename F, int RD, int RS, bool DEEP = false>
__global__ __launch_bounds__(k12_threads<F>()) void k_grad_xyz_c(const T* __restrict__ Ic, const F* __restrict__ D0,
                                                             int zin0, int nzc, int ny, int nx, DevTaps<F> tp,
                                                             F* __restrict__ G, size_t fs, int zg0, int q0, int nq,
                                                             int zc, int ntile, int nbx) {
    constexpr int TY = K12_TY, TX = k12_tx<F, RD>(), NRW = TY + 2 * RD, CW = k12_cw<F>();
    constexpr int NWX = k12_nwx<F>(), NWV = NWX * TY;  // waves per row; per block
    constexpr int NR = 2 * RD + 2, NRS = RD + 1, AP = k12_ap<F>();  // ring slots; A tile pitch
    constexpr bool ODD = k12_odd<F>();
    constexpr int AF = (ODD ? 2 : 1) * TY * AP, AB = 3 * AF;  // A field stride (even [+ odd] copy), buffer stride
    static_assert(NRS >= 2 * RS + 1 && NR % NRS == 0 && NR % 2 == 0 && TX >= 8, "K12 geometry");
    constexpr int EF = 16 / (int)sizeof(F), ET = 16 / (int)sizeof(T);  // elements per granule
    constexpr int GD = CW / EF + 1, GI = CW / ET + 1;                   // granules per staged row
    constexpr int NG = NRW * (GD + GI), NJ = (NG + 63) / 64;            // granules / DMA instrs per plane
    constexpr int K = k12_k<T, F, RD>();  // planes per DMA chunk
    constexpr int NCH = k12_nch<T, F, RD, DEEP>();  // chunks of slots (DMA issued NCH - 1 chunks ahead)
    constexpr int SLOT = k12_slot_bytes<T, F, RD>(), NSLOT = NCH * K;
    static_assert(k12_lds_bytes<T, F, RD, DEEP>() <= 160 * 1024, "K12 LDS");
    constexpr int NJW = (NJ + NWV - 1) / NWV;                           // DMA instrs per wave per plane
    constexpr int NJMIN = NJ / NWV;  // ... on the waves with the fewest (NJW - 1 or NJW)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    F* At = reinterpret_cast<F*>(smem_raw + NSLOT * SLOT);  // [2 buffers][3 fields][even, odd][TY][AP]
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    // (row role, column part) of wave w, as rp = role * NWX + part: fp64 spreads the roles' work
    // evenly over the SIMDs (wave w runs on SIMD w % 4; roles 0 / 1 / 2 / 3 do 180 / 180 / 132 /
    // 104 fp64 ops per step): SIMDs get roles {0,0,3} {1,1,3} {0,2,3} {1,2,2} instead of {0,1,2}
    // {0,1,3} {0,2,3} {1,2,3} (busiest SIMD 464 instead of 492 ops per step).  Same box: c3 K12
    // 0.445 / 0.447 -> 0.435 / 0.438 ms, c4 3.26 -> 3.22, c2 0.089 -> 0.087 (profiles/r05/ab_k12_perm/)
    const int rp = NWX == 3 ? (int)((0x8ba976415230ull >> (4 * w)) & 15u) : w;
    const int role = rp / NWX, c = 64 * (rp % NWX) + lane;
    const int per = (ntile + 7) >> 3;
    const int tile = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (tile >= ntile) return;  // block-uniform
    const int by = tile / nbx, bx = tile - by * nbx;
    const int y0 = by * TY, x0 = bx * TX;
    const int qa = q0 + (int)blockIdx.y * zc, nout = min(zc, q0 + nq - qa);
    const size_t plane = (size_t)ny * nx;
    // staged columns: dt0 from gd0, I from gi0 (granule-aligned starts of the block's window)
    const int xs = max(x0 - RD, 0);
    const int gd0 = xs / EF * EF, gi0 = xs / ET * ET;
    const int gc = clampi(x0 - RD + c, 0, nx - 1);  // this thread's staged column (y passes)
    const int pd = gc - gd0, pi = gc - gi0;         // its LDS positions in the dt0 / I rows
    // DMA sources of this wave's instructions (plane-relative element offsets): instruction
    // j = w + NWV i covers granules 64 j .. 64 j + 63 of the slot (dt0 rows, then I rows)
    unsigned doff[NJW];
    bool isd[NJW];
#pragma unroll
    for (int i = 0; i < NJW; ++i) {
        const int g = min(64 * (w + NWV * i) + lane, NG - 1);
        if (g < NRW * GD) {
            const int r = g / GD, q = g - r * GD;
            isd[i] = true;
            doff[i] = (unsigned)clampi(y0 - RD + r, 0, ny - 1) * (unsigned)nx + (unsigned)min(gd0 + q * EF, nx - EF);
        } else {
            const int gg = g - NRW * GD, r = gg / GI, q = gg - r * GI;
            isd[i] = false;
            doff[i] = (unsigned)clampi(y0 - RD + r, 0, ny - 1) * (unsigned)nx + (unsigned)min(gi0 + q * ET, nx - ET);
        }
    }
    const unsigned lds0 = (unsigned)(uintptr_t)smem_raw;
    const int nsteps = nout + 2 * RD;
    auto issue_plane = [&](int s) {  // DMA of step s's plane into slot s % NSLOT
        const size_t pz = (size_t)(clampi(qa - RD + s, 0, nzc - 1) - zin0) * plane;
        const unsigned sb = lds0 + (unsigned)((s % NSLOT) * SLOT);
#pragma unroll
        for (int i = 0; i < NJW; ++i) {
            if (w + NWV * i < NJ) {
                const void* src = isd[i] ? (const void*)(D0 + pz + doff[i]) : (const void*)(Ic + pz + doff[i]);
                glds16(src, __builtin_amdgcn_readfirstlane(sb + (unsigned)((w + NWV * i) * 1024)));
            }
        }
    };
    auto issue_chunk = [&](int m) {
        for (int s = m * K; s < min((m + 1) * K, nsteps); ++s) issue_plane(s);
    };
    F hg[RD + 1], hd[RD + 1], hs[RS + 1];
#pragma unroll
    for (int k = 0; k <= RD; ++k) hg[k] = tp.g[k], hd[k] = tp.d[k];
#pragma unroll
    for (int k = 0; k <= RS; ++k) hs[k] = tp.s[k];
    // x / z passes: output column x0 + c - RD (reads clamped into the block's outputs);
    // stores of lanes outside the volume are skipped
    const int cx = clampi(c, RD, RD + TX - 1);
    const int xo = x0 + c - RD, yo = y0 + role;
    const bool st_ok = c >= RD && c < RD + TX && xo < nx && yo < ny;
    constexpr unsigned ES = sizeof(F);
    const unsigned vout = (unsigned)(xo < 0 ? 0 : xo) * ES, sout = (unsigned)(yo < ny ? yo : 0) * (unsigned)nx * ES;
    F r1[NR], r2[NRS], r3[NRS], r4[NR];  // z rings of B1 .. B4
    // ---- y passes of step s (roles 0..2): staged rows of slot s % NSLOT -> A tile s & 1 ----
    auto ypass_step = [&](int s, int par) {
        F* A = At + par * AB;
        const unsigned char* slot = smem_raw + (s % NSLOT) * SLOT;
        auto ypass = [&]<int R, bool ANTI, bool DT>(const F(&h)[R + 1]) {
            F v[NRW];
            if constexpr (DT) {
                const F* rd_ = reinterpret_cast<const F*>(slot) + pd;
#pragma unroll
                for (int i = 0; i < NRW; ++i) {
                    v[i] = rd_[i * GD * EF];
                    // fp64: single ds_read_b64s, not pairs of rows in ds_read2_b64 (half rate)
                    if constexpr (k12_ysolo && sizeof(F) == 8) asm volatile("" ::: "memory");
                }
            } else {
                const T* ri_ = reinterpret_cast<const T*>(slot + NRW * GD * 16) + pi;
#pragma unroll
                for (int i = 0; i < NRW; ++i) v[i] = (F)ri_[i * GI * ET];
            }
            F* a = A + role * AF + c;  // even copy at c, odd copy at c - 1
#pragma unroll
            for (int r = 0; r < TY; ++r) {
                F o = v[r + RD] * h[0];
#pragma unroll
                for (int k = R; k >= 1; --k)
                    o = o + (ANTI ? (v[r + RD - k] - v[r + RD + k]) : (v[r + RD - k] + v[r + RD + k])) * h[k];
                a[r * AP] = o;
                // odd copy at c - 1; lane c = 0 writes the pad column AP - 1 of the row before
                // (even copy's last row for r = 0), which no window reads: no exec mask
                if constexpr (ODD) a[TY * AP + r * AP - 1] = o;
            }
        };
        if (role == 0)
            ypass.template operator()<RD, false, true>(hg);
        else if (role == 1)
            ypass.template operator()<RD, true, false>(hd);
        else if (role == 2)
            ypass.template operator()<RS, false, false>(hs);
    };
    // Schedule (one barrier per step; the y passes of step s + 1 run beside the x / z passes
    // of step s, in the other A buffer):
    //   prologue: chunk 0 loaded; chunk 1 issued; y(0)
    //   step s:   [last step of a chunk: vmcnt(0) — retires the next chunk's DMA, issued a
    //             chunk ago] barrier [then: issue the chunk after it into the slots of the
    //             chunk just finished] x / z (s), y (s + 1)
    // ---- z passes of step s (ring slot j = s mod NR): registers only ----
    auto zpass = [&](int s, auto jc) {
        constexpr int j = decltype(jc)::value;
        auto slotz = [](int i, int n) { return ((i % n) + n) % n; };
        if (s >= 2 * RD) {  // plane q = qa + s - 2 RD: dt and dz
            const int q = qa + s - 2 * RD;
            constexpr int cz = j - RD;
            F o1 = r1[slotz(cz, NR)] * hg[0], o4 = r4[slotz(cz, NR)] * hd[0];
#pragma unroll
            for (int k = RD; k >= 1; --k) {
                o1 = o1 + (r1[slotz(cz - k, NR)] + r1[slotz(cz + k, NR)]) * hg[k];
                o4 = o4 + (r4[slotz(cz - k, NR)] - r4[slotz(cz + k, NR)]) * hd[k];
            }
            if (NCH == 3 || st_ok) {  // NCH 3: every lane stores (vmcnt counts), others out of range
                const size_t pq = (size_t)(q - zg0) * plane;
                const unsigned vo = NCH == 3 && !st_ok ? 0x80000000u : vout;
                buf_st<F>(o1, buf_rsrc(G + pq), vo, sout);
                buf_st<F>(o4, buf_rsrc(G + 3 * fs + pq), vo, sout);
            }
        }
        if (s >= RD + RS && s < nout + RD + RS) {  // plane q = qa + s - RD - RS: dy and dx
            const int q = qa + s - RD - RS;
            constexpr int cz = j - RS;
            F o2 = r2[slotz(cz, NRS)] * hs[0], o3 = r3[slotz(cz, NRS)] * hs[0];
#pragma unroll
            for (int k = RS; k >= 1; --k) {
                o2 = o2 + (r2[slotz(cz - k, NRS)] + r2[slotz(cz + k, NRS)]) * hs[k];
                o3 = o3 + (r3[slotz(cz - k, NRS)] + r3[slotz(cz + k, NRS)]) * hs[k];
            }
            if (NCH == 3 || st_ok) {
                const size_t pq = (size_t)(q - zg0) * plane;
                const unsigned vo = NCH == 3 && !st_ok ? 0x80000000u : vout;
                buf_st<F>(o2, buf_rsrc(G + fs + pq), vo, sout);
                buf_st<F>(o3, buf_rsrc(G + 2 * fs + pq), vo, sout);
            }
        }
    };
    // NCH 3 (one-plane chunks): at step s plane s + 1 must have landed.  Issued at step s - 2
    // (right after that step's barrier); behind it this wave issued the stores of steps s - 2 and
    // s - 1 (unconditional: zst of them) and plane s + 2's loads (>= NJMIN): wait until at most
    // that many are left, rounded down to a few immediates (a smaller count only waits longer)
    auto zst = [&](int q) { return (q >= 2 * RD ? 2 : 0) + (q >= RD + RS && q < nout + RD + RS ? 2 : 0); };
    auto wait_plane = [&](int s) {
        const int cnt = zst(s - 2) + zst(s - 1) + (s + 2 < nsteps ? NJMIN : 0);
        if (cnt >= 8 + NJMIN)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 + NJMIN) : "memory");
        else if (cnt >= 4 + NJMIN)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + NJMIN) : "memory");
        else if (cnt >= NJMIN)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NJMIN) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    issue_chunk(0);
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int m = 1; m < NCH; ++m) issue_chunk(m);  // (clamped to nsteps)
    ypass_step(0, 0);
    for (int u0 = 0; u0 < nsteps; u0 += NR) {
        bool done = false;
        [&]<int... J>(std::integer_sequence<int, J...>) {
            (
                [&] {
                    if (done) return;
                    constexpr int j = J;
                    const int s = u0 + j;
                    const bool chunk_end = s % K == K - 1;
                    if (chunk_end) {
                        if constexpr (NCH == 3)
                            wait_plane(s);
                        else
                            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    lds_barrier();
                    if (chunk_end) {
                        const int m2 = s / K + NCH;
                        if (m2 * K < nsteps) issue_chunk(m2);
                    }
                    // k12_defer: the z passes of step s - 1 here, ahead of this step's x-window
                    // reads in program order: register-only work the scheduler can run while those
                    // LDS reads are in flight (their ring slots exclude slot j, written below)
                    if constexpr (k12_defer<F>())
                        if (s >= 1) zpass(s - 1, std::integral_constant<int, (j + NR - 1) % NR>{});
                    // ---- x passes: thread (row `role`, staged column cx) of A tile s & 1 ----
                    // window [cx - R, cx + R] of a field row, as 16-byte pairs from the copy
                    // where it starts aligned
                    const F* arow = At + (j & 1) * AB + role * AP;  // NR even: parity of s
                    auto window = [&]<int R>(int f, F (&x)[2 * R + 2]) {
                        const int st = cx - R;
                        if constexpr (!ODD) {  // single elements, one ds_read_b64 each
                            const F* q = arow + f * AF + st;
#pragma unroll
                            for (int i = 0; i <= 2 * R; ++i) {
                                x[i] = q[i];
                                asm volatile("" ::: "memory");  // no pairing into ds_read2_b64
                            }
                            return;
                        }
                        const F* q = arow + f * AF + ((st & 1) ? TY * AP + st - 1 : st);
                        typedef F F2 __attribute__((ext_vector_type(2)));
                        const F2* q2 = reinterpret_cast<const F2*>(__builtin_assume_aligned(q, 2 * sizeof(F)));
#pragma unroll
                        for (int i = 0; i <= R; ++i) {
                            const F2 v2 = q2[i];
                            x[2 * i] = v2.x;
                            x[2 * i + 1] = v2.y;
                        }
                    };
                    F b1, b2, b3, b4;
                    if constexpr (NWX == 3) {
                        // 12-wave blocks (168 VGPRs): one x window live at a time, each window's
                        // reads pinned behind the previous field's pass (3 waves per SIMD hide
                        // the three LDS round trips)
                        {
                            F x1[2 * RD + 2];
                            window.template operator()<RD>(0, x1);
                            b1 = x1[RD] * hg[0];
#pragma unroll
                            for (int k = RD; k >= 1; --k) b1 = b1 + (x1[RD - k] + x1[RD + k]) * hg[k];
                        }
                        asm volatile("" : "+v"(b1)::"memory");
                        {
                            F x3[2 * RD + 2];
                            window.template operator()<RD>(2, x3);
                            b3 = x3[RD] * hd[0], b4 = x3[RD] * hs[0];
#pragma unroll
                            for (int k = RD; k >= 1; --k) b3 = b3 + (x3[RD - k] - x3[RD + k]) * hd[k];
#pragma unroll
                            for (int k = RS; k >= 1; --k) b4 = b4 + (x3[RD - k] + x3[RD + k]) * hs[k];
                        }
                        asm volatile("" : "+v"(b3), "+v"(b4)::"memory");
                        {
                            F x2[2 * RS + 2];
                            window.template operator()<RS>(1, x2);
                            b2 = x2[RS] * hs[0];
#pragma unroll
                            for (int k = RS; k >= 1; --k) b2 = b2 + (x2[RS - k] + x2[RS + k]) * hs[k];
                        }
                    } else {
                        F x1[2 * RD + 2], x2[2 * RS + 2], x3[2 * RD + 2];
                        window.template operator()<RD>(0, x1);
                        window.template operator()<RS>(1, x2);
                        window.template operator()<RD>(2, x3);
                        b1 = x1[RD] * hg[0], b2 = x2[RS] * hs[0], b3 = x3[RD] * hd[0], b4 = x3[RD] * hs[0];
#pragma unroll
                        for (int k = RD; k >= 1; --k) {
                            b1 = b1 + (x1[RD - k] + x1[RD + k]) * hg[k];
                            b3 = b3 + (x3[RD - k] - x3[RD + k]) * hd[k];
                        }
#pragma unroll
                        for (int k = RS; k >= 1; --k) {
                            b2 = b2 + (x2[RS - k] + x2[RS + k]) * hs[k];
                            b4 = b4 + (x3[RD - k] + x3[RD + k]) * hs[k];
                        }
                    }
                    r1[j % NR] = b1;
                    r4[j % NR] = b4;
                    r2[j % NRS] = b2;
                    r3[j % NRS] = b3;
                    // ---- y passes of the next step (independent work for the scheduler) ----
                    if (s + 1 < nsteps) ypass_step(s + 1, (j + 1) & 1);
                    // ---- z passes (k12_defer: at the next step; the last step's here) ----
                    if (!k12_defer<F>() || s + 1 >= nsteps) zpass(s, std::integral_constant<int, j>{});
                    if (s + 1 >= nsteps) done = true;
                }(),
                ...);
        }(std::make_integer_sequence<int, NR>{});
        if (done) break;
    }
}

}  // namespace

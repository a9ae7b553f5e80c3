#pragma once
// of3d_common.hpp — device code that every flow kernel family of libof3d shares: limits, tap and
// frame tables, the 1-D pass helpers, buffer and LDS helpers, and the tile layout more than one
// family uses.  Each family has a header of its own (of3d_k0.hpp, of3d_grad.hpp, of3d_k12.hpp,
// of3d_k34.hpp, of3d_solve.hpp, of3d_k5.hpp, of3d_general.hpp) that a unit includes
// only where it instantiates that family; the kernel templates are instantiated only in the
// unit that takes their address (kt_*.hip getters, of3d_host.hip for the small kernels).
//
//
// Re-design (not a port) of the hot path of ScientistRachel/OpticalFlow3D_dev
// src/Python/calc_flow.py:175-360 (calc_flow3D) and :18-173 (calc_flow2D).
// The reference runs 40 scipy.ndimage.correlate1d passes over full fp64
// volumes plus a per-voxel LAPACK cgeev; here the same arithmetic is a
// five-kernel device pipeline over HBM-resident fields:
//
//   K0c tderiv   : temporal derivative of the centre frame (T2)
//   K1c grad_xy  : y and x passes of the four gradient filters (T4), column march:
//                  register rings down each column, LDS tiles for the x pass
//   K2c grad_z   : z pass of the four gradients (T4), z march with register rings
//   K34 prod_wyx : the 9 (2D: 5) structure-tensor products + W y (register ring)
//                  + W x (LDS tiles) in one pass (T5); the plan autotunes its shape
//   K5c wz_solve : W z pass (T5, LDS-DMA windows) + closed-form 3x3 solve (T6) +
//                  fp64 smallest eigenvalue (T7);  2D: 2x2 solve + rel (T8)
//
// The earlier kernels (k_tderiv_vec, k_grad_xy, k_grad_z, k_prod_wy + k_wx,
// k_wz_solve_dma / k_wz_solve) remain for radii and input types without a
// compiled column-march instance, and as the A/B reference (bit-identical).
//
// Bit-exactness: every 1-D pass evaluates scipy's NI_Correlate1D order for
// (anti)symmetric taps  o = c0*w0; for k=r..1: o += (c[-k] +- c[+k]) * w[-k]
// with indices clamped to the GLOBAL volume edge at every pass
// (mode='nearest'); products and the solve copy calc_flow.py's expression
// trees.  Built with -ffp-contract=off (no FMA) and IEEE div/sqrt.
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace {

constexpr int kMaxR = 48;          // largest supported tap radius (LDS tiles)
constexpr int kMaxT = 2 * 32 + 1;  // largest temporal window (rt <= 32)
constexpr double kEps = 2.220446049250313e-16;  // np.finfo(float).eps, calc_flow.py:155,338

// Half taps on the device: h[0] = centre tap w[r], h[k] = w[r-k] (left side),
// exactly the coefficients scipy multiplies by in the symmetric branch.
// F = the arithmetic type of the filter passes: double (exact mode) or float
// (OF3D_FP32 plans); taps are stored in F.
template <typename F>
struct DevTaps {
    const F* g;  // gauss   (rd)
    const F* d;  // deriv   (rd, antisymmetric)
    const F* s;  // smooth  (rs)
    const F* t;  // tderiv  (rt, antisymmetric)
    const F* w;  // window  (rw)
    // step-order copies (hr[q] = w[q], q < r, then kTapPad zeros), see lds_pass
    const F *gr, *dr, *sr, *tr, *wr;
    int rd, rs, rt, rw;
};

struct Frames {
    const void* p[kMaxT];  // frames c-rt .. c+rt
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename T, typename F>
__device__ __forceinline__ F ldf(const void* p, size_t i) {
    return (F)(reinterpret_cast<const T*>(p)[i]);
}

// 1-D pass over a staged LDS line, R consecutive outputs per thread at line
// positions base..base+R-1 (elements `st` doubles apart); the staged line
// already holds the clamped halo (positions base-r .. base+R-1+r valid).
// Summation order per output is scipy's: o = c*w0; k = r..1: o += (lo +- hi)*w.
//
// Register reuse without register moves: at step q (k = r-q) output i needs
// lo = s[base-r+q+i] and hi = s[base+r-q+i].  Both are streams indexed by
// (q+i) and (q-i); each lives in a ring of M slots (L[m % M], U[m % M]), and
// the q loop is unrolled by M so every slot index is a compile-time constant.
// Per step: 2 LDS reads, 3R fp64 ops, ~3R live doubles, any radius.
// Weights: h[0] is the centre tap; hr[q] = h[r - q] = w[q] is the weight of step
// q (outermost tap first), padded with kTapPad zeros past hr[r - 1].  PRE: each
// M-step block takes its M weights with one uniform load issued a block ahead
// (no scalar load + wait inside the steps; costs 2M registers, so kernels at
// their register cap keep PRE off).
constexpr int kTapPad = 8;  // >= the largest M

template <int R, bool ANTI, bool PRE = true, int D = 1, bool WRAP = false, typename F>
__device__ __forceinline__ void lds_pass(const F* __restrict__ s, int st, int base, const F* __restrict__ h,
                                         const F* __restrict__ hr, int r, F (&out)[R], int wmask = 0) {
    // WRAP: the staged line is a ring of (wmask + 1) positions (power of two)
    auto at = [&](int i) { return WRAP ? s[(i & wmask) * st] : s[i * st]; };
    // Ring of M = R + D - 1 slots per stream: the two reads issued after step q
    // are first consumed at step q + D (prefetch distance D hides LDS latency).
    constexpr int M = R + D - 1;
    static_assert(M <= kTapPad, "tap padding too short for this ring");
    F L[M], U[M];
#pragma unroll
    for (int i = 0; i < R; ++i) out[i] = at(base + i) * h[0];
#pragma unroll
    for (int m = 0; m < M; ++m) L[m] = at(base - r + m);           // S_lo[0 .. M-1]
#pragma unroll
    for (int m = -(R - 1); m < D; ++m) U[((m % M) + M) % M] = at(base + r - m);  // S_hi[-(R-1) .. D-1]
    F wb[M];  // weights of the current block
    if constexpr (PRE) {
#pragma unroll
        for (int m = 0; m < M; ++m) wb[m] = hr[m];
    }
    auto step = [&](int q, auto jc) {  // phase j = q mod M (compile-time)
        constexpr int j = decltype(jc)::value;
        const F wk = PRE ? wb[j] : hr[q];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const F lo = L[(j + i) % M];
            const F hi = U[((j - i) % M + M) % M];
            out[i] = out[i] + (ANTI ? (lo - hi) : (lo + hi)) * wk;
        }
        L[j] = at(base - r + q + M);           // S_lo[q+M]   (slot of S_lo[q], done)
        U[(j + D) % M] = at(base + r - q - D);  // S_hi[q+D]   (slot of S_hi[q-R+1], done)
    };
    int q = 0;
    for (; q + M <= r; q += M) {
        F wn[M];  // next block's weights, in flight during this block
        if constexpr (PRE) {
#pragma unroll
            for (int m = 0; m < M; ++m) wn[m] = hr[q + M + m];
        }
        [&]<int... J>(std::integer_sequence<int, J...>) {
            (step(q + J, std::integral_constant<int, J>{}), ...);
        }(std::make_integer_sequence<int, M>{});
        if constexpr (PRE) {
#pragma unroll
            for (int m = 0; m < M; ++m) wb[m] = wn[m];
        }
    }
    const int t = r - q;  // 0 .. M-1 remaining steps
    [&]<int... J>(std::integer_sequence<int, J...>) {
        ((J < t ? step(q + J, std::integral_constant<int, J>{}) : void()), ...);
    }(std::make_integer_sequence<int, M - 1>{});
}

// lds_pass with a compile-time radius RW and the half taps in registers
// (h[k] = w[RW - k]: uniform, so SGPRs): fully unrolled, no weight loads or
// waits inside the pass, same scipy order.  Stream rings as in lds_pass
// (prefetch distance D); reads past the last needed element are skipped.
// SOLO: every element read stays a single ds_read_b64 / _b32 (an empty fence after each): the
// compiler otherwise pairs reads one window row apart into ds_read2_b64, which moves 1 KiB per
// wave-instruction in 8 LDS cycles where two ds_read_b64 take 4 (MI355X_MICROARCH.md, LDS table)
template <int R, int RW, int D, bool ANTI = false, bool SOLO = false, typename F>
__device__ __forceinline__ void lds_pass_c(const F* __restrict__ s, int st, int base, const F (&h)[RW + 1],
                                           F (&out)[R]) {
    constexpr int M = R + D - 1;
    auto rd = [&](int i) {
        const F v = s[i * st];
        if constexpr (SOLO) asm volatile("" ::: "memory");
        return v;
    };
    F L[M], U[M];
#pragma unroll
    for (int i = 0; i < R; ++i) out[i] = rd(base + i) * h[0];
#pragma unroll
    for (int m = 0; m < M; ++m) L[m] = rd(base - RW + m);  // S_lo[0 .. M-1]
#pragma unroll
    for (int m = -(R - 1); m < D; ++m) U[((m % M) + M) % M] = rd(base + RW - m);  // S_hi[-(R-1) .. D-1]
#pragma unroll
    for (int q = 0; q < RW; ++q) {  // k = RW - q, outermost tap first
        const int j = q % M;
        const F wk = h[RW - q];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const F lo = L[(j + i) % M];
            const F hi = U[((j - i) % M + M) % M];
            out[i] = out[i] + (ANTI ? (lo - hi) : (lo + hi)) * wk;
        }
        if (q + M <= RW + R - 2) L[j] = rd(base - RW + q + M);  // S_lo[q+M]
        if (q + D <= RW - 1) U[(j + D) % M] = rd(base + RW - q - D);  // S_hi[q+D]
    }
}
// The wave-specialised K34's consumers read single elements (fp64: c3 K34 1.65 -> 1.60 ms, c4
// 10.93 -> 10.87, same box, profiles/r06/abk5/).  K5c keeps the compiler's ds_read2_b64 pairs: single
// reads there cost its CSE of the window's centre values (576 instead of 450 reads per field set)
// and measured slower (c3 K5c 0.978 -> 1.015 ms, c4 6.82 -> 6.97); so did the lockstep K34 forms
// (c2 K34 0.17 -> 0.19 ms)
constexpr bool k5c_solo64 = false;
template <typename F>
constexpr bool k5c_solo = sizeof(F) == 8 && k5c_solo64;
constexpr bool k34_solo = true;

// W-y tile row r starts at r cwp + 28 (r / 4): with cwp = 1 (mod 32) every row start is
// r mod 4 (mod 32) elements (bank-conflict-free phase B, see k_prod_wyx)
__host__ __device__ constexpr int k34_row(int r, int cwp) { return r * cwp + 28 * (r / 4); }
__host__ __device__ constexpr int k34_tile(int s, int cwp) { return s * cwp + 28 * (s / 4); }  // per tile buffer
// tile row pitch for a block of tx outputs: its 2 rw halo positions, = 1 (mod 32)
__host__ __device__ constexpr int k34_pitch(int tx, int rw) { return ((tx + 2 * rw + 31) & ~31) + 1; }

// value of lane `lane` (wave-uniform index) of a per-lane F, to every lane of the wave
template <typename F>
__device__ __forceinline__ F bcast_lane(F v, int lane) {
    if constexpr (sizeof(F) == 8) {
        const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)b, lane);
        const unsigned hi = __builtin_amdgcn_readlane((unsigned)(b >> 32), lane);
        return __builtin_bit_cast(F, ((unsigned long long)hi << 32) | lo);
    } else {
        return __builtin_bit_cast(F, __builtin_amdgcn_readlane(__builtin_bit_cast(unsigned, v), lane));
    }
}

__device__ __forceinline__ void lds_barrier() {
    // LDS-only barrier: global loads in flight stay in flight (__syncthreads
    // would also drain vmcnt, i.e. the phase-A prefetch)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Raw buffer access (one SGPR descriptor per plane-field, 32-bit SGPR row offset +
// one VGPR lane offset): no per-load 64-bit address VALU, no address VGPRs.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, 0x7fffffff, 0x00020000);
}
template <typename F>
__device__ __forceinline__ F buf_ld(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    if constexpr (sizeof(F) == 8)
        return __builtin_bit_cast(F, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
    else
        return __builtin_bit_cast(F, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
// Buffer stores with the default cache policy (non-temporal stores measured neutral: c3 fp64
// 3.707 vs 3.718 ms, c5 fp32 120.65 vs 120.76; every stored field is re-read by a later kernel).
constexpr int kStAux = 0;
template <typename F>
__device__ __forceinline__ void buf_st(F v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    if constexpr (sizeof(F) == 8)
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b64(r, 0, 0, 0)), v),
                                              r, voff, soff, kStAux);
    else
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, kStAux);
}
// N consecutive values from registers, as 16-byte stores (N * sizeof(F) a multiple of 16)
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
template <typename F, int N>
__device__ __forceinline__ void buf_st_n(const F (&v)[N], __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    constexpr int PER = 16 / (int)sizeof(F);
    if constexpr (N % PER != 0) {  // not whole 16-byte pieces: element stores
#pragma unroll
        for (int i = 0; i < N; ++i) buf_st<F>(v[i], r, voff + i * (unsigned)sizeof(F), soff);
        return;
    }
#pragma unroll
    for (int i = 0; i < N; i += PER) {
        F w[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) w[e] = v[i + e];
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, w), r, voff + i * (unsigned)sizeof(F), soff,
                                               kStAux);
    }
}
template <typename T>
__device__ __forceinline__ T buf_ld_raw(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    if constexpr (sizeof(T) == 1)
        return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b8(r, voff, soff, 0));
    else if constexpr (sizeof(T) == 2)
        return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0));
    else
        return buf_ld<T>(r, voff, soff);
}

// 16-byte global -> LDS copy (LDS-DMA): lane i's 16 bytes land at lds_byte + 16 i.
// Inline asm keeps it out of the compiler's wait bookkeeping (the compiler
// would drain it with vmcnt(0) before every LDS read); waits are explicit.
__device__ __forceinline__ void glds16(const void* src, unsigned lds_byte) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(lds_byte)
                 : "memory");
}

}  // namespace

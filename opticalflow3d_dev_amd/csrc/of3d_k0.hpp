#pragma once
// of3d_k0.hpp — K0: the temporal-derivative kernels (pipeline overview: of3d_common.hpp).
#include <type_traits>

#include "of3d_common.hpp"

namespace {

// ---------------------------------------------------------------------------
// K0: temporal derivative of the centre frame (T2, calc_flow.py:276-277):
//   dt0 = I[c]*T[0] + sum_{k=rt..1} (I[c-k] - I[c+k]) * T[k]
// (scipy's antisymmetric order, outer tap first; the reference filters all Nt
// frames and keeps the centre — only the centre line is formed here).
// Streaming, one voxel per lane; frames by stride (one stack) or pointer table.
// ---------------------------------------------------------------------------
template <typename T, typename F>
__global__ __launch_bounds__(256) void k_tderiv(Frames fr, long long fstride, size_t off0, size_t n, int rt,
                                                const F* __restrict__ ht, F* __restrict__ D0) {
    const size_t st = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += st) {
        const size_t idx = off0 + i;
        F c, dt;
        if (fstride) {
            const T* p = reinterpret_cast<const T*>(fr.p[0]) + idx;
            c = (F)p[(long long)rt * fstride];
            dt = c * ht[0];
            for (int k = rt; k >= 1; --k)
                dt = dt + ((F)p[(long long)(rt - k) * fstride] - (F)p[(long long)(rt + k) * fstride]) * ht[k];
        } else {
            c = ldf<T, F>(fr.p[rt], idx);
            dt = c * ht[0];
            for (int k = rt; k >= 1; --k)
                dt = dt + (ldf<T, F>(fr.p[rt - k], idx) - ldf<T, F>(fr.p[rt + k], idx)) * ht[k];
        }
        D0[i] = dt;
    }
}

// Vectorised K0 (any frame order, e.g. a device ring buffer; every frame
// aligned to the vector width): each lane handles V consecutive voxels with
// one 8- or 16-byte load per frame.
template <typename T>
struct K0Vec {
    static constexpr int V = sizeof(T) == 1 ? 8 : (sizeof(T) == 8 ? 2 : 4);
    static constexpr int B = V * (int)sizeof(T);  // 8 or 16 bytes
};

template <typename T, typename F>
__device__ __forceinline__ void load_vec(const T* p, F (&v)[K0Vec<T>::V]) {
    constexpr int V = K0Vec<T>::V;
    T t[V];
    if constexpr (K0Vec<T>::B == 8) {
        const unsigned long long raw = *reinterpret_cast<const unsigned long long*>(p);
        __builtin_memcpy(t, &raw, 8);
    } else {
        const uint4 raw = *reinterpret_cast<const uint4*>(p);
        __builtin_memcpy(t, &raw, 16);
    }
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = (F)t[i];
}

template <typename T, typename F>
__global__ __launch_bounds__(256) void k_tderiv_vec(Frames fr, size_t off0, size_t ngroups, int rt,
                                                    const F* __restrict__ ht, F* __restrict__ D0) {
    constexpr int V = K0Vec<T>::V;
    const size_t st = (size_t)gridDim.x * 256;
    for (size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += st) {
        const size_t o = off0 + gi * V;
        F c[V], a[V], b[V], dt[V];
        load_vec<T, F>(reinterpret_cast<const T*>(fr.p[rt]) + o, c);
#pragma unroll
        for (int i = 0; i < V; ++i) dt[i] = c[i] * ht[0];
        for (int k = rt; k >= 1; --k) {
            load_vec<T, F>(reinterpret_cast<const T*>(fr.p[rt - k]) + o, a);
            load_vec<T, F>(reinterpret_cast<const T*>(fr.p[rt + k]) + o, b);
            const F w = ht[k];
#pragma unroll
            for (int i = 0; i < V; ++i) dt[i] = dt[i] + (a[i] - b[i]) * w;
        }
        if constexpr (sizeof(F) == 8) {
            double2* d = reinterpret_cast<double2*>(D0 + gi * V);
#pragma unroll
            for (int i = 0; i < V / 2; ++i) d[i] = make_double2(dt[2 * i], dt[2 * i + 1]);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) D0[gi * V + i] = dt[i];
        }
    }
}

// K0 with a compile-time temporal radius: all 2RT+1 frame loads of a lane issued
// before the first use (the runtime-rt loop above keeps only two in flight per lane:
// latency-bound at 4.3 TB/s on c2).  Same arithmetic order.
// One vector group of K0c: voxels o .. o + V - 1 of every frame -> D0g[0 .. V - 1] (shared by
// the K0c kernel and the next-frame K0 inside the fused K5c, so both compute the same bits).
template <typename T, typename F, int RT>
__device__ __forceinline__ void k0_group_dt(const Frames& fr, size_t o, const F (&h)[RT + 1], F (&dt)[K0Vec<T>::V]) {
    constexpr int V = K0Vec<T>::V, NW = 2 * RT + 1;
    using Raw = typename std::conditional<K0Vec<T>::B == 8, unsigned long long, uint4>::type;
    Raw raw[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) raw[i] = *reinterpret_cast<const Raw*>(reinterpret_cast<const T*>(fr.p[i]) + o);
    auto val = [&](int i, int e) {
        T t[V];
        __builtin_memcpy(t, &raw[i], sizeof(Raw));
        return (F)t[e];
    };
#pragma unroll
    for (int e = 0; e < V; ++e) dt[e] = val(RT, e) * h[0];
#pragma unroll
    for (int k = RT; k >= 1; --k)
#pragma unroll
        for (int e = 0; e < V; ++e) dt[e] = dt[e] + (val(RT - k, e) - val(RT + k, e)) * h[k];
}
template <typename F, int V>
__device__ __forceinline__ void k0_store(const F (&dt)[V], F* __restrict__ D0g) {
    if constexpr (sizeof(F) == 8) {
        double2* d = reinterpret_cast<double2*>(D0g);
#pragma unroll
        for (int i = 0; i < V / 2; ++i) d[i] = make_double2(dt[2 * i], dt[2 * i + 1]);
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) D0g[i] = dt[i];
    }
}
template <typename T, typename F, int RT>
__device__ __forceinline__ void k0_group(const Frames& fr, size_t o, const F (&h)[RT + 1], F* __restrict__ D0g) {
    F dt[K0Vec<T>::V];
    k0_group_dt<T, F, RT>(fr, o, h, dt);
    k0_store<F, K0Vec<T>::V>(dt, D0g);
}

template <typename T, typename F, int RT>
__global__ __launch_bounds__(256) void k_tderiv_vec_c(Frames fr, size_t off0, size_t ngroups, const F* __restrict__ ht,
                                                      F* __restrict__ D0) {
    constexpr int V = K0Vec<T>::V;
    F h[RT + 1];
#pragma unroll
    for (int k = 0; k <= RT; ++k) h[k] = ht[k];
    const size_t st = (size_t)gridDim.x * 256;
    for (size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += st)
        k0_group<T, F, RT>(fr, off0 + gi * V, h, D0 + gi * V);
}

// K0 batching (of3d_plan_execute_ahead): the temporal derivatives of M consecutive output
// frames of a time series in one pass — frames c-rt .. c+M-1+rt, each loaded once (2rt + M
// loads for M derivatives instead of M (2rt + 1)); output m (centre c + m) in the order of
// k0_group_dt (bit-identical), to D0 + m * dstride.
template <typename T, typename F, int RT, int M>
__global__ __launch_bounds__(256) void k_tderiv_multi(Frames fr, size_t off0, size_t ngroups,
                                                      const F* __restrict__ ht, F* __restrict__ D0,
                                                      size_t dstride) {
    constexpr int V = K0Vec<T>::V, NW = 2 * RT + M;
    static_assert(NW <= kMaxT, "frame table");
    using Raw = typename std::conditional<K0Vec<T>::B == 8, unsigned long long, uint4>::type;
    F h[RT + 1];
#pragma unroll
    for (int k = 0; k <= RT; ++k) h[k] = ht[k];
    const size_t st = (size_t)gridDim.x * 256;
    for (size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x; gi < ngroups; gi += st) {
        const size_t o = off0 + gi * V;
        Raw raw[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) raw[i] = *reinterpret_cast<const Raw*>(reinterpret_cast<const T*>(fr.p[i]) + o);
        auto val = [&](int i, int e) {
            T t[V];
            __builtin_memcpy(t, &raw[i], sizeof(Raw));
            return (F)t[e];
        };
        F dt[M][V];
#pragma unroll
        for (int e = 0; e < V; ++e) {  // one voxel at a time: its NW frame values converted once
            F x[NW];
#pragma unroll
            for (int i = 0; i < NW; ++i) x[i] = val(i, e);
#pragma unroll
            for (int m = 0; m < M; ++m) {
                dt[m][e] = x[RT + m] * h[0];
#pragma unroll
                for (int k = RT; k >= 1; --k) dt[m][e] = dt[m][e] + (x[RT + m - k] - x[RT + m + k]) * h[k];
            }
        }
#pragma unroll
        for (int m = 0; m < M; ++m) k0_store<F, V>(dt[m], D0 + m * dstride + gi * V);
    }
}

// The NEXT frame's temporal derivative, computed inside the current frame's K5c (frame
// pipelining, of3d_plan_execute_next): the K0 stage is pure HBM streaming and K5c is VALU-bound,
// so its loads ride in K5c's memory slack instead of taking a launch of their own.
template <typename F>
struct K0Next {
    Frames fr;        // frames c-rt .. c+rt of the next output frame
    size_t off0;      // element offset of the first voxel (plane zb0) in each frame
    size_t ngroups;   // vector groups of K0Vec<T>::V voxels
    const F* ht;      // temporal taps h[0 .. rt]
    F* D0;            // its dt0 (the plan's dt0 field, origin zb0)
};

}  // namespace

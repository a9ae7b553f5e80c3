#pragma once
// radix_key.hpp — the key arithmetic of the radix selects (kt_summary.hip: of3d_quantile over a
// flat array; kt_relsel.hip: of3d_rel_select over a box, several ranks at once): the
// order-preserving unsigned image of a float, the 11-bit digits it is narrowed by, and the
// closing interpolation of two order statistics.  One statement, so the two selects cannot
// drift apart.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace of3dk {

using u64 = unsigned long long;

// key(v): the order-preserving unsigned image of the float bits (sign bit set: all bits
// flipped, else the sign bit set); -0.0 takes +0.0's key.  11-bit digits from the top:
// float32 11 + 11 + 10 bits (3 passes), float64 5 x 11 + 9 bits (6 passes).
constexpr int kDigit = 11, kBins = 1 << kDigit;
constexpr int kMaxPasses = 6;

template <typename T>
struct KeyOf;
template <>
struct KeyOf<float> {
    static constexpr int bits = 32, passes = 3;
    static __device__ __forceinline__ u64 key(float v) {
        unsigned u = __float_as_uint(v);
        if ((u << 1) == 0) u = 0;  // -0.0 -> +0.0
        return (u & 0x80000000u) ? (unsigned)~u : (u | 0x80000000u);
    }
    static __device__ __forceinline__ float value(u64 k) {
        const unsigned u = (unsigned)k;
        return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
    }
};
template <>
struct KeyOf<double> {
    static constexpr int bits = 64, passes = 6;
    static __device__ __forceinline__ u64 key(double v) {
        u64 u = (u64)__double_as_longlong(v);
        if ((u << 1) == 0) u = 0;
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double value(u64 k) {
        return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
    }
};

// digit p of a `bits`-wide key: [shift, shift + width)
__host__ __device__ constexpr int digit_shift(int bits, int p) {
    return bits - (p + 1) * kDigit > 0 ? bits - (p + 1) * kDigit : 0;
}
__host__ __device__ constexpr int digit_width(int bits, int p) {
    return bits - (p + 1) * kDigit >= 0 ? kDigit : bits - p * kDigit;
}

// numpy's _lerp of the order statistics a <= b in the array's dtype (gamma: the weight of b).
// lo == hi: b == a and the same expression gives a — or NaN for an infinite a, as numpy's
template <typename T>
__device__ __forceinline__ T select_lerp(T a, T b, double gamma) {
    const T g1 = (T)gamma;
    const T diff = b - a;
    return g1 < (T)0.5 ? a + diff * g1 : b - diff * ((T)1 - g1);
}

}  // namespace of3dk

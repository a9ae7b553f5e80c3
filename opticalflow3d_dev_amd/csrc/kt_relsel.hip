// kt_relsel.hip — how the reliability threshold is formed (no reference kernel counterpart: the
// reference's figure scripts crop the saved rel TIFF and call prctile / np.percentile on the
// host, plot_figure5.m:80-84, plot_figure3_ROIfigures.m:70-84, plot_figureS3_reliability.ipynb
// cells 4-8): of3d_rel_select, up to 8 percentiles of one box of the volume read in place, and
// of3d_rel_profile, per ROI the counts above each threshold and the histogram of rel.  Both are
// stream-ordered end to end: nothing returns to the host, the select's outputs stay in device
// memory for every pass that takes a d_thresh.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "radix_key.hpp"
#include "summary_dev.hpp"

namespace {

using of3dk::u64, of3dk::kBins, of3dk::kMaxPasses, of3dk::KeyOf, of3dk::digit_shift, of3dk::digit_width;

// ---------------------------------------------------------------------------
// Box select.  of3d_quantile's radix select (kt_summary.hip) with two things new: the walk over
// a box's rows, and up to 16 ranks (two per percentile) narrowed at once.  One histogram is kept
// per GROUP, a distinct key prefix among the ranks: pass 0 has one group; after each pass
// k_rs_pick sorts the distinct narrowed prefixes, so a voxel finds its group by a range reject
// and a short binary search, and after pass 0 most voxels match none.  A rank value that occurs
// twice always shares its group, so the host knows a bound G on the groups (the distinct rank
// values, rounded up to a power of two): the histogram kernel is instantiated for G = 1 (pass
// 0), 2, 4, 8, 16, with G x 2048 x 4 B of LDS — 8 KiB to 128 KiB of the CU's 160 KiB; at G = 16
// one 512-thread workgroup per CU, at G <= 2 of3d_quantile's footprint.  Which instance runs
// is a function of the host arguments alone.
// ---------------------------------------------------------------------------
constexpr int kRsThreads = 512, kRsWaves = kRsThreads / 64;
constexpr int kPickThreads = 256;
constexpr int kMaxQ = OF3D_SELECT_MAX, kMaxRanks = 2 * kMaxQ;
constexpr int kChunkVecs = 256;  // 16-byte vectors a wave takes per work item: 64 lanes x 4

struct RsState {
    u64 prefix[kMaxRanks];  // the key bits fixed so far
    u64 rank[kMaxRanks];    // the rank within the prefix
    u64 gp[kMaxRanks];      // the groups of the coming pass: distinct prefixes >> its `up`, ascending
    int rg[kMaxRanks];      // the group of rank r
    int ng, pad;
    u64 n_nan;
};
constexpr size_t kRsStateBytes = (sizeof(RsState) + 255) / 256 * 256;
constexpr size_t kRsBytes = kRsStateBytes + (size_t)kMaxPasses * kMaxRanks * kBins * sizeof(u64);

struct RsRanks {
    u64 rank[kMaxRanks];  // lo, hi of percentile k at 2k, 2k + 1
    double gamma[kMaxQ];
    int n_q;
};

// The box as rows of contiguous voxels: full-width rows of a plane are one row, full planes too
// (the whole volume is one row).  Row r starts at base + (r / dyr) * stride_z + (r % dyr) * stride_y.
struct RsBox {
    long long rows, row_len, dyr, stride_z, stride_y, base;
    long long cpr;  // work items (chunks of kChunkVecs vectors) per row
};

template <typename T, int G>
__global__ __launch_bounds__(kRsThreads) void k_rs_hist(const T* __restrict__ a, RsBox B, int pass,
                                                        RsState* __restrict__ st, u64* __restrict__ hist) {
    __shared__ unsigned h[G * kBins];
    __shared__ u64 s_gp[kMaxRanks];
    __shared__ unsigned nan_s;
    const int ng = pass ? (st->ng < G ? st->ng : G) : 1;
    for (int i = threadIdx.x; i < ng * kBins; i += kRsThreads) h[i] = 0;
    if ((int)threadIdx.x < ng) s_gp[threadIdx.x] = pass ? st->gp[threadIdx.x] : 0;
    if (threadIdx.x == 0) nan_s = 0;
    __syncthreads();
    constexpr int bits = KeyOf<T>::bits;
    const int shift = digit_shift(bits, pass), width = digit_width(bits, pass);
    const unsigned mask = (1u << width) - 1;
    const int up = shift + width;  // the bits above the digit are the prefix (none in pass 0)
    const u64 gmin = s_gp[0], gmax = s_gp[ng - 1];
    unsigned nans = 0;
    auto count = [&](T v) {
        const u64 k = KeyOf<T>::key(v);
        nans += v != v;
        const u64 top = pass ? k >> up : 0;
        if (top < gmin || top > gmax) return;
        const unsigned d = (unsigned)(k >> shift) & mask;
        if constexpr (G == 1) {
            atomicAdd(&h[d], 1u);
        } else {
            int lo = 0, hi = ng;  // s_gp[lo] <= top
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (top >= s_gp[mid])
                    lo = mid;
                else
                    hi = mid;
            }
            if (s_gp[lo] == top) atomicAdd(&h[lo * kBins + d], 1u);
        }
    };
    // a wave per work item: 16-byte loads over the aligned middle of the row, element loads for
    // the row's head and tail (item 0 of the row)
    constexpr int V = 16 / (int)sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const int lane = threadIdx.x & 63;
    const long long items = B.rows * B.cpr;
    const long long nwaves = (long long)gridDim.x * kRsWaves;
    for (long long it = (long long)blockIdx.x * kRsWaves + (threadIdx.x >> 6); it < items; it += nwaves) {
        const long long r = it / B.cpr, c = it - r * B.cpr;
        const T* p = a + B.base + (r / B.dyr) * B.stride_z + (r % B.dyr) * B.stride_y;
        const long long mis = (long long)(((uintptr_t)p % 16) / sizeof(T));
        const long long head = mis ? (V - mis < B.row_len ? V - mis : B.row_len) : 0;
        const long long nvec = (B.row_len - head) / V;
        const long long rest = B.row_len - head - nvec * V;  // < V
        if (c == 0) {
            if (lane < head) count(p[lane]);
            if (lane < rest) count(p[head + nvec * V + lane]);
        }
        const vec_t* pv = reinterpret_cast<const vec_t*>(p + head);
        const long long v0 = c * kChunkVecs + lane;
        vec_t v[kChunkVecs / 64];
        bool in[kChunkVecs / 64];
#pragma unroll
        for (int u = 0; u < kChunkVecs / 64; ++u) {
            in[u] = v0 + 64 * u < nvec;
            if (in[u]) v[u] = pv[v0 + 64 * u];
        }
#pragma unroll
        for (int u = 0; u < kChunkVecs / 64; ++u) {
            if (!in[u]) continue;
#pragma unroll
            for (int j = 0; j < V; ++j) count(v[u][j]);
        }
    }
    if (pass == 0 && nans) atomicAdd(&nan_s, nans);
    __syncthreads();
    u64* g = hist + (size_t)pass * kMaxRanks * kBins;
    for (int i = threadIdx.x; i < ng * kBins; i += kRsThreads) {
        const unsigned c = h[i];
        if (c) atomicAdd(&g[i], (u64)c);
    }
    if (pass == 0 && threadIdx.x == 0 && nan_s) atomicAdd(&st->n_nan, (u64)nan_s);
}

// One workgroup: per rank the bin of its group's histogram that holds it, the narrowed prefix and
// the rank within the bin; then the groups of the coming pass, or after the last pass (the
// prefixes are the order statistics' keys) the interpolations.
template <typename T>
__global__ __launch_bounds__(kPickThreads) void k_rs_pick(int pass, RsState* __restrict__ st,
                                                          const u64* __restrict__ hist, RsRanks R,
                                                          T* __restrict__ out) {
    constexpr int per = kBins / kPickThreads;
    constexpr int bits = KeyOf<T>::bits;
    __shared__ u64 part[kPickThreads];
    __shared__ u64 res[kMaxRanks][2];
    const int shift = digit_shift(bits, pass);
    const int nr = 2 * R.n_q;
    const u64* g = hist + (size_t)pass * kMaxRanks * kBins;
    for (int r = 0; r < nr; ++r) {
        const u64* hr = g + (size_t)(pass ? st->rg[r] : 0) * kBins;
        const u64 rank = st->rank[r];
        u64 c[per], s = 0;
        for (int j = 0; j < per; ++j) {
            c[j] = hr[threadIdx.x * per + j];
            s += c[j];
        }
        part[threadIdx.x] = s;
        __syncthreads();
        for (int off = 1; off < kPickThreads; off <<= 1) {  // inclusive scan of the threads' counts
            const u64 v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += v;
            __syncthreads();
        }
        u64 before = part[threadIdx.x] - s;
        for (int j = 0; j < per; ++j) {
            if (rank >= before && rank < before + c[j]) {
                res[r][0] = (u64)(threadIdx.x * per + j);
                res[r][1] = rank - before;
            }
            before += c[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        u64 pf[kMaxRanks];
        for (int r = 0; r < nr; ++r) {
            pf[r] = st->prefix[r] | (res[r][0] << shift);
            st->prefix[r] = pf[r];
            st->rank[r] = res[r][1];
        }
        if (pass == KeyOf<T>::passes - 1) {
            for (int k = 0; k < R.n_q; ++k) {
                T v = of3dk::select_lerp<T>(KeyOf<T>::value(pf[2 * k]), KeyOf<T>::value(pf[2 * k + 1]), R.gamma[k]);
                if (st->n_nan) v = (T)__builtin_nan("");
                out[k] = v;
            }
        } else {
            // the coming pass's `up` is this pass's shift: its groups are the distinct pf >> shift
            u64 gp[kMaxRanks];
            int ng = 0;
            for (int r = 0; r < nr; ++r) {
                const u64 key = pf[r] >> shift;
                int i = 0;
                while (i < ng && gp[i] < key) ++i;
                if (i == ng || gp[i] != key) {
                    for (int j = ng; j > i; --j) gp[j] = gp[j - 1];
                    gp[i] = key;
                    ++ng;
                }
            }
            for (int r = 0; r < nr; ++r) {
                const u64 key = pf[r] >> shift;
                int i = 0;
                while (gp[i] != key) ++i;
                st->rg[r] = i;
            }
            for (int i = 0; i < ng; ++i) st->gp[i] = gp[i];
            st->ng = ng;
        }
    }
}

__global__ void k_rs_init(RsState* st, RsRanks R) {
    const int r = threadIdx.x;
    if (r < kMaxRanks) {
        st->prefix[r] = 0;
        st->rank[r] = r < 2 * R.n_q ? R.rank[r] : 0;
        st->gp[r] = 0;
        st->rg[r] = 0;
    }
    if (r == 0) st->ng = 1;
}

template <typename T>
int select_launch(const void* a, const RsBox& B, int64_t n_box, const RsRanks& R, int G, void* out, void* ws,
                  hipStream_t s) {
    RsState* st = (RsState*)ws;
    u64* hist = (u64*)((char*)ws + kRsStateBytes);
    OF3DK_HIP(hipMemsetAsync(ws, 0, kRsStateBytes + (size_t)KeyOf<T>::passes * kMaxRanks * kBins * sizeof(u64), s));
    hipLaunchKernelGGL(k_rs_init, dim3(1), dim3(64), 0, s, st, R);
    // 16 elements per thread and pass at least; fewer workgroups where each flushes more bins
    const int64_t want = (n_box + (int64_t)kRsThreads * 16 - 1) / ((int64_t)kRsThreads * 16);
    const int64_t item_wgs = (B.rows * B.cpr + kRsWaves - 1) / kRsWaves;
    auto blocks = [&](int g) {
        const int64_t cap = g <= 2 ? 1024 : (g <= 8 ? 512 : 256);
        int64_t b = want < item_wgs ? want : item_wgs;
        b = b > cap ? cap : b;
        return (unsigned)(b < 1 ? 1 : b);
    };
    for (int p = 0; p < KeyOf<T>::passes; ++p) {
        const int g = p ? G : 1;
#define OF3D_RS_LAUNCH(GG)                                                                                       \
    hipLaunchKernelGGL((k_rs_hist<T, GG>), dim3(blocks(GG)), dim3(kRsThreads), 0, s, (const T*)a, B, p, st, hist)
        switch (g) {
            case 1: OF3D_RS_LAUNCH(1); break;
            case 2: OF3D_RS_LAUNCH(2); break;
            case 4: OF3D_RS_LAUNCH(4); break;
            case 8: OF3D_RS_LAUNCH(8); break;
            default: OF3D_RS_LAUNCH(16); break;
        }
#undef OF3D_RS_LAUNCH
        hipLaunchKernelGGL(k_rs_pick<T>, dim3(1), dim3(kPickThreads), 0, s, p, st, (const u64*)hist, R, (T*)out);
    }
    OF3DK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// Profile.  Grid (kSumMaxBlocks, n_roi), the summary's partition and walk (plan_boxes,
// box_share).  Per voxel: NaN?, rel > t_k in rel's dtype for the n_q thresholds, and the bin of
// (double)rel among the edges of the result's head.  Integer counts only: per-thread counters,
// a shuffle tree per wave, LDS atomics, then 64-bit integer atomics into the zeroed result — a
// box's words do not depend on the other boxes and are the same on every run.
// ---------------------------------------------------------------------------
using of3dk::kSumThreads, of3dk::kMaxBins, of3dk::kMaxRoi;
constexpr int kRpHead = OF3D_PROFILE_HEAD;  // n_roi, n_q, nbins
constexpr int kRpCounters = 1 + kMaxQ;      // n_nan, n_above[k]

struct RpParams : of3dk::BoxParams {
    int n_q, nbins;
    int head_words;  // kRpHead + n_q + nbins + 1
    int roi_words;   // 2 + n_q + nbins
};

// The head: n_roi, n_q, nbins, the thresholds as float64, and with `range` the edges
// np.linspace(lo, hi, nbins + 1) of np.histogram's outer edges (lo == hi widened by 0.5 to both
// sides; a non-finite end: NaN edges, which take no value)
template <typename T>
__global__ void k_rp_head(u64* __restrict__ result, const T* __restrict__ thr, const T* __restrict__ range, int n_roi,
                          int n_q, int nbins) {
    const int i = threadIdx.x;
    if (i == 0) result[0] = (u64)n_roi, result[1] = (u64)n_q, result[2] = (u64)nbins;
    if (i < n_q) result[kRpHead + i] = (u64)__double_as_longlong((double)thr[i]);
    if (range && i <= nbins) {
        double lo = (double)range[0], hi = (double)range[1], e;
        if (!(__builtin_isfinite(lo) && __builtin_isfinite(hi))) {
            e = __builtin_nan("");
        } else {
            if (lo == hi) lo -= 0.5, hi += 0.5;
            const double delta = hi - lo, step = delta / (double)nbins;
            // multiply, then add (no contraction); a step that underflowed to 0: linspace's other order
            e = step == 0.0 ? ((double)i / (double)nbins) * delta + lo : (double)i * step + lo;
            if (i == nbins) e = hi;
        }
        result[kRpHead + n_q + i] = (u64)__double_as_longlong(e);
    }
}

__device__ __forceinline__ unsigned wave_sum_u(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <typename T>
__global__ __launch_bounds__(kSumThreads) void k_rp_boxes(const T* __restrict__ rel, const T* __restrict__ thr_p,
                                                          RpParams P, u64* __restrict__ result) {
    const int roi = blockIdx.y, nb = P.nb[roi];
    if ((int)blockIdx.x >= nb) return;
    __shared__ double edges[kMaxBins + 1];
    __shared__ unsigned hist[kMaxBins];
    __shared__ unsigned cnt_s[kRpCounters];
    const double* edges_g = reinterpret_cast<const double*>(result + kRpHead + P.n_q);
    for (int i = threadIdx.x; i <= P.nbins; i += kSumThreads) edges[i] = edges_g[i];
    for (int i = threadIdx.x; i < P.nbins; i += kSumThreads) hist[i] = 0;
    if (threadIdx.x < kRpCounters) cnt_s[threadIdx.x] = 0;
    __syncthreads();

    T thr[kMaxQ];
#pragma unroll
    for (int k = 0; k < kMaxQ; ++k) thr[k] = k < P.n_q ? thr_p[k] : (T)__builtin_nan("");  // v > NaN: never
    of3dk::BoxShare sh = of3dk::box_share(P, roi, nb);
    const long long count = sh.count;
    unsigned cnt[kRpCounters];
#pragma unroll
    for (int k = 0; k < kRpCounters; ++k) cnt[k] = 0;

    constexpr int U = 4;
    for (long long e = threadIdx.x; e < count; e += (long long)U * kSumThreads) {
        T fr[U];
        bool in[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            in[u] = e + (long long)u * kSumThreads < count;
            fr[u] = (T)0;
            if (in[u]) fr[u] = rel[sh.index()];
            sh.w.advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!in[u]) continue;
            const T v = fr[u];
            cnt[0] += v != v;
#pragma unroll
            for (int k = 0; k < kMaxQ; ++k) cnt[1 + k] += v > thr[k];
            const int b = of3dk::find_bin(edges, P.nbins, (double)v);
            if (b >= 0) atomicAdd(&hist[b], 1u);
        }
    }

#pragma unroll
    for (int k = 0; k < kRpCounters; ++k) {
        const unsigned v = wave_sum_u(cnt[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&cnt_s[k], v);
    }
    __syncthreads();
    u64* rr = result + P.head_words + (size_t)roi * P.roi_words;
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int* bx = P.box[roi];
        rr[0] = (u64)((long long)(bx[1] - bx[0]) * (bx[3] - bx[2]) * (bx[5] - bx[4]));
    }
    if ((int)threadIdx.x < 1 + P.n_q && cnt_s[threadIdx.x]) atomicAdd(&rr[1 + threadIdx.x], (u64)cnt_s[threadIdx.x]);
    of3dk::flush_hist(hist, P.nbins, rr + 2 + P.n_q);
}

bool profile_sizes_ok(int n_roi, int n_q, int nbins) {
    return n_roi >= 1 && n_roi <= kMaxRoi && n_q >= 0 && n_q <= kMaxQ && nbins >= 1 && nbins <= kMaxBins;
}

}  // namespace

extern "C" {

size_t of3d_rel_select_workspace_bytes(int rel_f64) {
    (void)rel_f64;
    return kRsBytes;
}

int of3d_rel_select(const void* d_rel, int rel_f64, int64_t nz, int64_t ny, int64_t nx, const int64_t* box, int n_q,
                    const int64_t* lo, const int64_t* hi, const double* gamma, void* d_out, void* workspace,
                    void* stream) {
    if (!d_rel || !lo || !hi || !gamma || !d_out || !workspace) return of3dk::set_error("of3d: null argument");
    if (nz < 1 || ny < 1 || nx < 1 || nz > INT32_MAX || ny > INT32_MAX || nx > INT32_MAX)
        return of3dk::set_error("of3d: select dims must lie in [1, 2^31)");
    if (nz > (INT64_MAX / 4) / ny / nx) return of3dk::set_error("of3d: select volume too large (2^61 voxels)");
    if (n_q < 1 || n_q > kMaxQ) return of3dk::set_error("of3d: 1 to 8 percentiles per select");
    const int64_t dims[3] = {nz, ny, nx};
    const int64_t whole[6] = {0, nz, 0, ny, 0, nx};
    const int64_t* b = box ? box : whole;
    int64_t ext[3];
    for (int a = 0; a < 3; ++a)
        if ((ext[a] = of3dk::box_extent(b, 0, a, dims)) < 0) return -1;
    const int64_t n_box = ext[0] * ext[1] * ext[2];
    RsRanks R{};
    R.n_q = n_q;
    int distinct = 0;
    for (int k = 0; k < n_q; ++k) {
        if (lo[k] < 0 || lo[k] > hi[k] || hi[k] > n_box - 1)
            return of3dk::set_error("of3d: select ranks must satisfy 0 <= lo <= hi <= n_box-1");
        if (!(gamma[k] >= 0.0 && gamma[k] <= 1.0)) return of3dk::set_error("of3d: select gamma must lie in [0, 1]");
        R.rank[2 * k] = (u64)lo[k], R.rank[2 * k + 1] = (u64)hi[k];
        R.gamma[k] = gamma[k];
    }
    for (int r = 0; r < 2 * n_q; ++r) {
        bool seen = false;
        for (int q = 0; q < r; ++q) seen |= R.rank[q] == R.rank[r];
        distinct += !seen;
    }
    int G = 1;
    while (G < distinct) G <<= 1;
    RsBox B{};
    B.base = (b[0] * ny + b[2]) * nx + b[4];
    if (ext[2] == nx && ext[1] == ny) {
        B.rows = 1, B.row_len = n_box, B.dyr = 1, B.stride_z = 0, B.stride_y = 0;
    } else if (ext[2] == nx) {
        B.rows = ext[0], B.row_len = ext[1] * nx, B.dyr = 1, B.stride_z = ny * nx, B.stride_y = 0;
    } else {
        B.rows = ext[0] * ext[1], B.row_len = ext[2], B.dyr = ext[1], B.stride_z = ny * nx, B.stride_y = nx;
    }
    const int64_t V = rel_f64 ? 2 : 4;
    B.cpr = (B.row_len / V + kChunkVecs - 1) / kChunkVecs;
    if (B.cpr < 1) B.cpr = 1;
    hipStream_t s = (hipStream_t)stream;
    return rel_f64 ? select_launch<double>(d_rel, B, n_box, R, G, d_out, workspace, s)
                   : select_launch<float>(d_rel, B, n_box, R, G, d_out, workspace, s);
}

size_t of3d_rel_profile_result_bytes(int n_roi, int n_q, int nbins) {
    if (!profile_sizes_ok(n_roi, n_q, nbins)) return 0;
    return ((size_t)kRpHead + n_q + nbins + 1 + (size_t)n_roi * (2 + n_q + nbins)) * 8;
}

int of3d_rel_profile(const void* d_rel, int rel_f64, int64_t nz, int64_t ny, int64_t nx, const int64_t* rois,
                     int n_roi, const void* d_thresh, int n_q, int nbins, const double* edges, const void* d_range,
                     void* d_result, void* stream) {
    if (!d_rel || !rois || !d_result || (n_q > 0 && !d_thresh)) return of3dk::set_error("of3d: null argument");
    if (nz < 1 || ny < 1 || nx < 1 || nz > INT32_MAX || ny > INT32_MAX || nx > INT32_MAX)
        return of3dk::set_error("of3d: profile dims must lie in [1, 2^31)");
    if (n_roi < 1 || n_roi > kMaxRoi) return of3dk::set_error("of3d: 1 to 16 ROI boxes");
    if (n_q < 0 || n_q > kMaxQ) return of3dk::set_error("of3d: 0 to 8 thresholds per profile");
    if (nbins < 1 || nbins > kMaxBins) return of3dk::set_error("of3d: 1 to 256 bins of rel");
    if (!edges == !d_range) return of3dk::set_error("of3d: profile edges come either from the host or from d_range");
    RpParams P{};
    const int64_t dims[3] = {nz, ny, nx};
    if (of3dk::plan_boxes(rois, n_roi, dims, 0, P.nb) != 0) return -1;
    const int max_nb = of3dk::fill_boxes(P, dims, rois, n_roi);
    P.n_q = n_q, P.nbins = nbins;
    P.head_words = kRpHead + n_q + nbins + 1, P.roi_words = 2 + n_q + nbins;
    double host_edges[kMaxBins + 1];
    if (edges) {
        int nb1, eoff, hoff;
        const double* const ep[1] = {edges};
        if (of3dk::plan_hists<1>(&nbins, ep, &nb1, &eoff, &hoff, host_edges) < 0) return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    u64* res = (u64*)d_result;
    OF3DK_HIP(hipMemsetAsync(d_result, 0, of3d_rel_profile_result_bytes(n_roi, n_q, nbins), s));
    if (edges) of3dk::put_edges(s, (double*)(res + kRpHead + n_q), host_edges, nbins + 1);
    auto launch = [&](auto rt) {
        using RT = decltype(rt);
        hipLaunchKernelGGL(k_rp_head<RT>, dim3(1), dim3(320), 0, s, res, (const RT*)d_thresh, (const RT*)d_range, n_roi,
                           n_q, nbins);
        hipLaunchKernelGGL(k_rp_boxes<RT>, dim3(max_nb, n_roi), dim3(kSumThreads), 0, s, (const RT*)d_rel,
                           (const RT*)d_thresh, P, res);
    };
    rel_f64 ? launch(double{}) : launch(float{});
    OF3DK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// kt_summary.hip — device-side frame summaries (no reference kernel counterpart: the reference
// reduces its saved TIFFs on the host, example_analysis_script.ipynb cells 4-6 and the figure
// scripts): an exact order-statistic select (of3d_quantile) and the masked ROI sums and
// histograms of one frame (of3d_flow_summary).  Both are stream-ordered end to end: nothing
// returns to the host, the threshold stays in device memory between the two.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/of3d.h"
#include "kernels.hpp"
#include "radix_key.hpp"
#include "summary_dev.hpp"

namespace {

using u64 = unsigned long long;

// ---------------------------------------------------------------------------
// Radix select over radix_key.hpp's keys and 11-bit digits (float32 3 passes, float64 6).
// Both ranks are narrowed at once: each carries its own key prefix and remaining rank; while
// the prefixes agree one histogram serves both.
// ---------------------------------------------------------------------------
using of3dk::kDigit, of3dk::kBins, of3dk::kMaxPasses, of3dk::KeyOf, of3dk::digit_shift, of3dk::digit_width;  // radix_key.hpp
constexpr int kSelThreads = 256;

// workspace: state, then one histogram pair per pass (zeroed once per call)
struct SelState {
    u64 prefix[2];
    u64 rank[2];
    u64 n_nan;
    u64 pad[3];
};
constexpr size_t kSelHistWords = (size_t)kMaxPasses * 2 * kBins;
constexpr size_t kSelBytes = sizeof(SelState) + kSelHistWords * sizeof(u64);

template <typename T>
__global__ __launch_bounds__(kSelThreads) void k_sel_hist(const T* __restrict__ a, size_t n, int pass,
                                                          SelState* __restrict__ st, u64* __restrict__ hist) {
    __shared__ unsigned h[2][kBins];
    __shared__ unsigned nan_s;
    for (int i = threadIdx.x; i < 2 * kBins; i += kSelThreads) (&h[0][0])[i] = 0;
    if (threadIdx.x == 0) nan_s = 0;
    __syncthreads();
    constexpr int bits = KeyOf<T>::bits;
    const int shift = digit_shift(bits, pass), width = digit_width(bits, pass);
    const unsigned mask = (1u << width) - 1;
    const int up = shift + width;  // the bits above the digit are the prefix (none in pass 0)
    const u64 p0 = pass ? st->prefix[0] >> up : 0, p1 = pass ? st->prefix[1] >> up : 0;
    const bool two = p0 != p1;
    unsigned nans = 0;
    auto count = [&](T v) {
        const u64 k = KeyOf<T>::key(v);
        const u64 top = pass ? k >> up : 0;
        const unsigned d = (unsigned)(k >> shift) & mask;
        if (top == p0) atomicAdd(&h[0][d], 1u);
        if (two && top == p1) atomicAdd(&h[1][d], 1u);
        nans += v != v;
    };
    // 16-byte loads over the aligned middle of the array, element loads for its head and tail
    constexpr int V = 16 / (int)sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const size_t mis = ((uintptr_t)a % 16) / sizeof(T);
    const size_t head = mis ? (V - mis < n ? V - mis : n) : 0;
    const size_t nvec = (n - head) / V;
    const vec_t* av = reinterpret_cast<const vec_t*>(a + head);
    const size_t stride = (size_t)gridDim.x * kSelThreads, first = (size_t)blockIdx.x * kSelThreads + threadIdx.x;
    for (size_t i = first; i < nvec; i += stride) {
        const vec_t v = av[i];
#pragma unroll
        for (int j = 0; j < V; ++j) count(v[j]);
    }
    const size_t rest = n - head - nvec * V;  // < V
    if (first < head) count(a[first]);
    if (first >= head && first < head + rest) count(a[head + nvec * V + (first - head)]);
    if (pass == 0 && nans) atomicAdd(&nan_s, nans);
    __syncthreads();
    u64* g = hist + (size_t)pass * 2 * kBins;
    for (int i = threadIdx.x; i < 2 * kBins; i += kSelThreads) {
        const unsigned c = (&h[0][0])[i];
        if (c) atomicAdd(&g[i], (u64)c);
    }
    if (pass == 0 && threadIdx.x == 0 && nan_s) atomicAdd(&st->n_nan, (u64)nan_s);
}

// One workgroup: the bin holding each rank, the narrowed prefix and the rank within the bin;
// after the last pass the prefixes are the two order statistics' keys -> the interpolation.
template <typename T>
__global__ __launch_bounds__(kSelThreads) void k_sel_pick(int pass, SelState* __restrict__ st,
                                                          const u64* __restrict__ hist, double gamma,
                                                          T* __restrict__ out) {
    constexpr int per = kBins / kSelThreads;
    constexpr int bits = KeyOf<T>::bits;
    __shared__ u64 part[kSelThreads];
    __shared__ u64 res[2][2];
    const int shift = digit_shift(bits, pass), width = digit_width(bits, pass);
    const int up = shift + width;
    const bool two = pass && (st->prefix[0] >> up) != (st->prefix[1] >> up);
    const u64* g = hist + (size_t)pass * 2 * kBins;
    for (int r = 0; r < 2; ++r) {
        const u64* hr = g + ((r && two) ? kBins : 0);
        const u64 rank = st->rank[r];
        u64 c[per], s = 0;
        for (int j = 0; j < per; ++j) {
            c[j] = hr[threadIdx.x * per + j];
            s += c[j];
        }
        part[threadIdx.x] = s;
        __syncthreads();
        for (int off = 1; off < kSelThreads; off <<= 1) {  // inclusive scan of the threads' counts
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
        u64 pf[2];
        for (int r = 0; r < 2; ++r) {
            pf[r] = st->prefix[r] | (res[r][0] << shift);
            st->prefix[r] = pf[r];
            st->rank[r] = res[r][1];
        }
        if (pass == KeyOf<T>::passes - 1) {
            // numpy's _lerp in the array's dtype (method 'linear')
            T v = of3dk::select_lerp<T>(KeyOf<T>::value(pf[0]), KeyOf<T>::value(pf[1]), gamma);
            if (st->n_nan) v = (T)__builtin_nan("");
            *out = v;
        }
    }
}

__global__ void k_sel_init(SelState* st, u64 lo, u64 hi) {
    st->prefix[0] = st->prefix[1] = 0;
    st->rank[0] = lo;
    st->rank[1] = hi;
}

template <typename T>
int quantile_launch(const void* a, int64_t n, int64_t lo, int64_t hi, double gamma, void* out, void* ws,
                    hipStream_t s) {
    SelState* st = (SelState*)ws;
    u64* hist = (u64*)((char*)ws + sizeof(SelState));
    OF3DK_HIP(hipMemsetAsync(ws, 0, kSelBytes, s));
    hipLaunchKernelGGL(k_sel_init, dim3(1), dim3(1), 0, s, st, (u64)lo, (u64)hi);
    // 16 elements per thread and pass at least; at most 2048 workgroups
    const int64_t want = (n + (int64_t)kSelThreads * 16 - 1) / ((int64_t)kSelThreads * 16);
    const unsigned blocks = (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    for (int p = 0; p < KeyOf<T>::passes; ++p) {
        hipLaunchKernelGGL(k_sel_hist<T>, dim3(blocks), dim3(kSelThreads), 0, s, (const T*)a, (size_t)n, p, st, hist);
        hipLaunchKernelGGL(k_sel_pick<T>, dim3(1), dim3(kSelThreads), 0, s, p, st, (const u64*)hist, gamma,
                           (T*)out);
    }
    OF3DK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------
// Frame summary.  Grid (kSumMaxBlocks, n_roi); workgroup b of a box walks rows
// [b*R/nb, (b+1)*R/nb) of the box's R = dz*dy rows, nb = a function of the box size alone.
// Per voxel k_flow_stats' arithmetic (of3d_general.hpp); sums in registers, a fixed shuffle tree
// over the lanes, the waves' partials added in wave order, one workspace slot per workgroup;
// k_sum_final adds a box's slots in index order.  Counts and histograms: LDS integer atomics,
// then 64-bit integer atomics into the (zeroed) result.  No floating-point atomics: the same
// inputs give the same bits on every run, and a box's row does not depend on the other boxes.
// ---------------------------------------------------------------------------
using of3dk::kSumThreads, of3dk::kSumWaves, of3dk::kSumMaxBlocks, of3dk::kMaxBins, of3dk::kMaxRoi;  // summary_host.hpp
constexpr int kNSum = 8;                   // mag x y z sin cos mag*sin mag*cos
constexpr int kNQ = OF3D_SUMMARY_QUANTITIES;
constexpr int kHead = of3dk::kSummaryHead, kRoiHead = of3dk::kSummaryRoiHead;  // result words before the boxes / before a box's histograms
static_assert(kRoiHead == 2 + kNSum);
constexpr size_t kSumSlotBytes = (size_t)kMaxRoi * kSumMaxBlocks * kNSum * sizeof(double);
constexpr size_t kEdgeWords = (size_t)kNQ * (kMaxBins + 1);
constexpr size_t kSumWsBytes = kSumSlotBytes + kEdgeWords * sizeof(double);

struct SumParams : of3dk::BoxParams {
    int nbins[kNQ];
    int eoff[kNQ];  // first edge of the quantity in the workspace's edge array
    int hoff[kNQ];  // first bin of the quantity in a box's histogram words
    int roi_words;  // result words per box
    double sxy, sz, st;
};

using of3dk::find_bin;  // summary_dev.hpp, shared with kt_axes.hip

// Masked: the mask factor of a voxel is bit `roi` of keep (of3d_mask_open) instead of rel > thr
template <typename VT, typename RelT, bool Masked>
__global__ __launch_bounds__(kSumThreads) void k_sum_boxes(const VT* __restrict__ vx, const VT* __restrict__ vy,
                                                           const VT* __restrict__ vz, const RelT* __restrict__ rel,
                                                           const RelT* __restrict__ thr_p,
                                                           const uint16_t* __restrict__ keep, SumParams P,
                                                           const double* __restrict__ edges_g,
                                                           double* __restrict__ slots, u64* __restrict__ result) {
    const int roi = blockIdx.y, nb = P.nb[roi];
    if ((int)blockIdx.x >= nb) return;
    __shared__ double edges[kEdgeWords];
    __shared__ unsigned hist[kNQ * kMaxBins];
    __shared__ unsigned nvalid_s;
    __shared__ double wsum[kSumWaves][kNSum];
    int ntot = 0, ne = 0;
    for (int q = 0; q < kNQ; ++q) {
        ntot += P.nbins[q];
        ne += P.nbins[q] ? P.nbins[q] + 1 : 0;
    }
    for (int i = threadIdx.x; i < ne; i += kSumThreads) edges[i] = edges_g[i];
    for (int i = threadIdx.x; i < ntot; i += kSumThreads) hist[i] = 0;
    if (threadIdx.x == 0) nvalid_s = 0;
    __syncthreads();

    of3dk::BoxShare sh = of3dk::box_share(P, roi, nb);
    // the threshold is read (and reported by k_sum_final) with a keep volume too
    const of3dk::FlowFields<VT, RelT, Masked> F{vx,    vy,   vz,   rel, keep,         (double)*thr_p,
                                                P.sxy, P.sz, P.st, roi, vz != nullptr};
    double acc[kNSum] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned nvalid = 0;

    of3dk::for_valid_voxels(F, sh, [&](const of3dk::Voxel& v, unsigned, unsigned, unsigned) {
        const double vxp = v.vxp, vyp = v.vyp, vzp = v.vzp;
        const double mag = sqrt(v.sq), h = sqrt(v.xy2);
        const double sn = vyp / h, cs = vxp / h;
        ++nvalid;
        acc[0] += mag;
        acc[1] += vxp;
        acc[2] += vyp;
        acc[3] += vzp;
        acc[4] += sn;
        acc[5] += cs;
        acc[6] += mag * sn;
        acc[7] += mag * cs;
        auto put = [&](int q, double x) {
            const int b = find_bin(edges + P.eoff[q], P.nbins[q], x);
            if (b >= 0) atomicAdd(&hist[P.hoff[q] + b], 1u);
        };
        if (P.nbins[0]) put(0, vxp);
        if (P.nbins[1]) put(1, vyp);
        if (P.nbins[2]) put(2, vzp);
        if (P.nbins[3]) put(3, mag);
        if (P.nbins[4]) put(4, atan2(vyp, vxp));
        if (P.nbins[5]) put(5, atan(vzp / h));
    });

    if (nvalid) atomicAdd(&nvalid_s, nvalid);
    of3dk::reduce_to_slot(acc, wsum, slots + ((size_t)roi * kSumMaxBlocks + blockIdx.x) * kNSum);
    u64* rr = result + kHead + (size_t)roi * P.roi_words;
    if (threadIdx.x == 0 && nvalid_s) atomicAdd(&rr[0], (u64)nvalid_s);
    of3dk::flush_hist(hist, ntot, rr + kRoiHead);
}

// One workgroup per box: its slots staged in LDS, then added in index order.
template <typename RelT>
__global__ __launch_bounds__(of3dk::kFinalThreads) void k_sum_final(const double* __restrict__ slots,
                                                                    const RelT* __restrict__ thr_p, SumParams P,
                                                                    u64* __restrict__ result) {
    __shared__ double s[kSumMaxBlocks * kNSum];
    const int roi = blockIdx.x;
    u64* rr = result + kHead + (size_t)roi * P.roi_words;
    of3dk::add_slots<kNSum, kNSum>(slots + (size_t)roi * kSumMaxBlocks * kNSum, P.nb[roi], s, rr + 2);
    if (threadIdx.x == 0) {
        const int* bx = P.box[roi];
        rr[1] = (u64)((long long)(bx[1] - bx[0]) * (bx[3] - bx[2]) * (bx[5] - bx[4]));
        if (roi == 0) {
            result[0] = (u64)__double_as_longlong((double)*thr_p);
            result[1] = (u64)P.n_roi;
            for (int q = 0; q < kNQ; ++q) result[2 + q] = (u64)P.nbins[q];
        }
    }
}

int roi_words(const int* nbins) { return kRoiHead + of3dk::total_bins<kNQ>(nbins); }

}  // namespace

extern "C" {

size_t of3d_quantile_workspace_bytes(int is_f64) {
    (void)is_f64;
    return kSelBytes;
}

int of3d_quantile(const void* a, int is_f64, int64_t n, int64_t lo, int64_t hi, double gamma, void* out,
                  void* workspace, void* stream) {
    if (!a || !out || !workspace) return of3dk::set_error("of3d: null argument");
    if (n < 1) return of3dk::set_error("of3d: quantile of an empty array");
    if (lo < 0 || lo > hi || hi > n - 1) return of3dk::set_error("of3d: quantile ranks must satisfy 0 <= lo <= hi <= n-1");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return of3dk::set_error("of3d: quantile gamma must lie in [0, 1]");
    hipStream_t s = (hipStream_t)stream;
    return is_f64 ? quantile_launch<double>(a, n, lo, hi, gamma, out, workspace, s)
                  : quantile_launch<float>(a, n, lo, hi, gamma, out, workspace, s);
}

size_t of3d_flow_summary_result_bytes(int n_roi, const int* nbins) {
    if (n_roi < 1 || n_roi > kMaxRoi || !of3dk::bins_ok<kNQ>(nbins)) return 0;
    return ((size_t)kHead + (size_t)n_roi * roi_words(nbins)) * 8;
}

size_t of3d_flow_summary_workspace_bytes(void) { return kSumWsBytes; }

static int summary_launch(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                          int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                          double tscale, const int64_t* rois, int n_roi, const int* nbins,
                          const double* const* edges, void* d_result, void* workspace, void* stream,
                          const uint16_t* keep, bool masked) {
    if (!vx || !vy || !rel || !d_thresh || !rois || !d_result || !workspace || (masked && !keep))
        return of3dk::set_error("of3d: null argument");
    if (of3dk::check_volume(nz, ny, nx, !vz) != 0) return -1;
    if (n_roi < 1 || n_roi > kMaxRoi) return of3dk::set_error("of3d: 1 to 16 ROI boxes");
    if (!of3dk::bins_ok<kNQ>(nbins)) return of3dk::set_error("of3d: 0 to 256 bins per quantity");
    if (!vz && (nbins[2] || nbins[5])) return of3dk::set_error("of3d: vz and phi histograms need a 3D volume");
    SumParams P{};
    P.sxy = xyscale, P.sz = zscale, P.st = tscale;
    const int64_t dims[3] = {nz, ny, nx};
    if (of3dk::plan_boxes(rois, n_roi, dims, 0, P.nb) != 0) return -1;
    const int max_nb = of3dk::fill_boxes(P, dims, rois, n_roi);
    double host_edges[kEdgeWords];
    const int eo = of3dk::plan_hists<kNQ>(nbins, edges, P.nbins, P.eoff, P.hoff, host_edges);
    if (eo < 0) return -1;
    P.roi_words = roi_words(nbins);
    hipStream_t s = (hipStream_t)stream;
    double* slots = (double*)workspace;
    double* d_edges = (double*)((char*)workspace + kSumSlotBytes);
    OF3DK_HIP(hipMemsetAsync(d_result, 0, of3d_flow_summary_result_bytes(n_roi, nbins), s));
    of3dk::put_edges(s, d_edges, host_edges, eo);
    of3dk::with_flow_types(v_f32, rel_f64, masked, [&](auto vt, auto rt, auto masked_c) {
        using VT = decltype(vt);
        using RT = decltype(rt);
        constexpr bool M = decltype(masked_c)::value;
        hipLaunchKernelGGL((k_sum_boxes<VT, RT, M>), dim3(max_nb, n_roi), dim3(kSumThreads), 0, s,
                           (const VT*)vx, (const VT*)vy, (const VT*)vz, (const RT*)rel, (const RT*)d_thresh, keep, P,
                           (const double*)d_edges, slots, (u64*)d_result);
        hipLaunchKernelGGL(k_sum_final<RT>, dim3(n_roi), dim3(of3dk::kFinalThreads), 0, s, (const double*)slots,
                           (const RT*)d_thresh, P, (u64*)d_result);
    });
    OF3DK_HIP(hipGetLastError());
    return 0;
}

int of3d_flow_summary(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                      int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                      double tscale, const int64_t* rois, int n_roi, const int* nbins, const double* const* edges,
                      void* d_result, void* workspace, void* stream) {
    return summary_launch(vx, vy, vz, rel, v_f32, rel_f64, nz, ny, nx, d_thresh, xyscale, zscale, tscale, rois, n_roi,
                          nbins, edges, d_result, workspace, stream, nullptr, false);
}

int of3d_flow_summary_masked(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                             int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                             double tscale, const int64_t* rois, int n_roi, const int* nbins,
                             const double* const* edges, void* d_result, void* workspace, void* stream,
                             const uint16_t* d_keep) {
    return summary_launch(vx, vy, vz, rel, v_f32, rel_f64, nz, ny, nx, d_thresh, xyscale, zscale, tscale, rois, n_roi,
                          nbins, edges, d_result, workspace, stream, d_keep, true);
}

}  // extern "C"

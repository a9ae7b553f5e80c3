#pragma once
// summary_host.hpp — the host side shared by the device-side summary passes (kt_summary.hip,
// kt_ccl.hip, kt_axes.hip, kt_whist.hip, kt_pair.hip, kt_quiver.hip, kt_contract.hip, kt_spread.hip,
// kt_relsel.hip, kt_export.hip): one statement of the volume check, the box check, the workgroup plan, the
// histogram plan with its edge validation, the edge upload and the dispatch over the field types.
// The entry points keep their own order of argument checks; what a check tests and says is here.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>

#include "../../include/of3d.h"
#include "kernels.hpp"

namespace of3dk {

constexpr int kMaxRoi = OF3D_SUMMARY_MAX_ROI, kMaxBins = OF3D_SUMMARY_MAX_BINS;

// of3d_flow_summary's result (include/of3d.h): the words before the boxes, and a box's words
// before its histograms (n_valid, n_voxels, the eight sums).  kt_summary.hip writes by them,
// kt_spread.hip finds a box's count and sums by them.
constexpr int kSummaryHead = 8, kSummaryRoiHead = 10;

// The workgroup partition of a box's reduction (k_sum_boxes, k_proj_boxes, k_whist_boxes, k_pair_boxes): workgroup b of nb
// walks rows [b*R/nb, (b+1)*R/nb) of the box's R = dz*dy rows.  nb is a function of the box
// alone (never of the device), so the summation order is fixed.
constexpr int kSumThreads = 512, kSumWaves = kSumThreads / 64;
constexpr int kSumMaxBlocks = 1024;        // workgroups (workspace slots) per box at most
constexpr int64_t kSumVoxPerBlock = 8192;  // a workgroup's share of a box at least
inline int64_t sum_workgroups(int64_t vox, int64_t rows) {
    int64_t nb = (vox + kSumVoxPerBlock - 1) / kSumVoxPerBlock;
    nb = nb > kSumMaxBlocks ? kSumMaxBlocks : nb;
    return nb > rows ? rows : nb;
}

// ---------------------------------------------------------------------------
// The volume and the field types of a flow pass
// ---------------------------------------------------------------------------
// dims in [1, 2^31); flat (the pass has no vz): a single plane
inline int check_volume(int64_t nz, int64_t ny, int64_t nx, bool flat) {
    if (nz < 1 || ny < 1 || nx < 1 || nz > INT32_MAX || ny > INT32_MAX || nx > INT32_MAX)
        return set_error("of3d: summary dims must lie in [1, 2^31)");
    if (flat && nz != 1) return set_error("of3d: a 2D summary (vz NULL) needs nz == 1");
    return 0;
}

// f(VT{}, RelT{}, std::bool_constant<Masked>{}) for the velocity type, the rel type and the
// mask source of a call: the box kernels' template arguments, chosen once
template <typename F>
void with_flow_types(int v_f32, int rel_f64, bool masked, F&& f) {
    auto with_mask = [&](auto vt, auto rt) {
        if (masked)
            f(vt, rt, std::true_type{});
        else
            f(vt, rt, std::false_type{});
    };
    if (v_f32)
        rel_f64 ? with_mask(float{}, double{}) : with_mask(float{}, float{});
    else
        rel_f64 ? with_mask(double{}, double{}) : with_mask(double{}, float{});
}

// ---------------------------------------------------------------------------
// Boxes
// ---------------------------------------------------------------------------
inline int check_roi_count(const int64_t* rois, int n_roi) {
    if (!rois) return set_error("of3d: null argument");
    if (n_roi < 1 || n_roi > kMaxRoi) return set_error("of3d: 1 to 16 ROI boxes");
    return 0;
}

// Axis a (0 z, 1 y, 2 x) of box r (z0 z1 y0 y1 x0 x1) lies in the volume: 0 <= b0 < b1 <= dims[a]
// (dims NULL: 2^31 - 1).  Returns its extent, 1 to 2^31 - 1, or -1 with the error set.
inline int64_t box_extent(const int64_t* rois, int r, int a, const int64_t* dims) {
    const int64_t b0 = rois[r * 6 + 2 * a], b1 = rois[r * 6 + 2 * a + 1];
    if (b0 < 0 || b0 >= b1 || b1 > (dims ? dims[a] : (int64_t)INT32_MAX))
        return set_error(("of3d: ROI " + std::to_string(r) + " is empty or outside the volume").c_str());
    return b1 - b0;
}

// The boxes of a reduction pass as of3d_flow_summary validates them (dims NULL: against 2^31
// alone) and their workgroups: box r's bounds, then box r's size, box by box.  nb_out[r]: the
// workgroups of box r.  For the passes with per-workgroup workspace slots (of3d_flow_whist,
// of3d_flow_pair, of3d_flow_spread) soff_out[r]: the first slot word of box r, slot_words: the sum over the boxes
// of workgroups * wg_words.  The three outputs may be NULL.
inline int plan_boxes(const int64_t* rois, int n_roi, const int64_t* dims, int wg_words = 0, int* nb_out = nullptr,
                      long long* soff_out = nullptr, size_t* slot_words = nullptr) {
    if (check_roi_count(rois, n_roi) != 0) return -1;
    size_t words = 0;
    for (int r = 0; r < n_roi; ++r) {
        int64_t ext[3];
        for (int a = 0; a < 3; ++a)
            if ((ext[a] = box_extent(rois, r, a, dims)) < 0) return -1;
        // a function of the box alone (never of the device): the summation order is fixed
        const int64_t rows = ext[0] * ext[1];  // < 2^62
        const int64_t big = INT64_MAX / 2;     // stands for any larger voxel count: the cap decides
        const int64_t nb = sum_workgroups(ext[2] > big / rows ? big : rows * ext[2], rows);
        // a workgroup's share, at most ceil(rows / nb) rows of ext[2] voxels, must stay below lim
        const int64_t lim = ((int64_t)1 << 31) - 4 * kSumThreads;
        if ((rows + nb - 1) / nb >= (lim + ext[2] - 1) / ext[2])
            return set_error("of3d: ROI too large (2^31 voxels per workgroup)");
        if (nb_out) nb_out[r] = (int)nb;
        if (soff_out) soff_out[r] = (long long)words;
        words += (size_t)nb * wg_words;
    }
    if (slot_words) *slot_words = words;
    return 0;
}

// What every box kernel takes of the volume and the boxes; SumParams, AxParams, WhParams and
// PairParams begin with it.
struct BoxParams {
    int nz, ny, nx, n_roi;
    int box[kMaxRoi][6];  // z0 z1 y0 y1 x0 x1
    int nb[kMaxRoi];      // workgroups of the box (plan_boxes)
};

// dims and the (validated) boxes into B, whose nb plan_boxes has filled; the largest nb (the
// grid's x), 1 at least
inline int fill_boxes(BoxParams& B, const int64_t dims[3], const int64_t* rois, int n_roi) {
    B.nz = (int)dims[0], B.ny = (int)dims[1], B.nx = (int)dims[2], B.n_roi = n_roi;
    int max_nb = 1;
    for (int r = 0; r < n_roi; ++r) {
        for (int a = 0; a < 6; ++a) B.box[r][a] = (int)rois[r * 6 + a];
        max_nb = B.nb[r] > max_nb ? B.nb[r] : max_nb;
    }
    return max_nb;
}

// ---------------------------------------------------------------------------
// Histograms of N quantities
// ---------------------------------------------------------------------------
template <int N>
bool bins_ok(const int* nbins) {
    if (!nbins) return false;
    for (int q = 0; q < N; ++q)
        if (nbins[q] < 0 || nbins[q] > kMaxBins) return false;
    return true;
}

template <int N>
int total_bins(const int* nbins) {
    int n = 0;
    for (int q = 0; q < N; ++q) n += nbins[q];
    return n;
}

// edges of the requested quantities: nbins + 1 each
template <int N>
int edge_words(const int* nbins) {
    int n = 0;
    for (int q = 0; q < N; ++q) n += nbins[q] ? nbins[q] + 1 : 0;
    return n;
}

// The edges of the requested quantities validated and packed one array after the other into
// host_edges (N * (kMaxBins + 1) words); eoff[q] / hoff[q]: the first edge / the first bin of
// quantity q among them.  Returns the number of edges, -1 on an error.
template <int N>
int plan_hists(const int* nbins, const double* const* edges, int* nbins_out, int* eoff, int* hoff,
               double* host_edges) {
    int eo = 0, ho = 0;
    for (int q = 0; q < N; ++q) {
        nbins_out[q] = nbins[q], eoff[q] = eo, hoff[q] = ho;
        if (!nbins[q]) continue;
        if (!edges || !edges[q]) return set_error("of3d: bins requested without edges");
        for (int i = 0; i <= nbins[q]; ++i) {
            const double e = edges[q][i];
            if (!(e == e) || (i && !(e > edges[q][i - 1])))
                return set_error("of3d: bin edges must ascend strictly and hold no NaN");
            host_edges[eo + i] = e;
        }
        eo += nbins[q] + 1, ho += nbins[q];
    }
    return eo;
}

// ---------------------------------------------------------------------------
// Edge upload: the edges travel as kernel arguments, stream-ordered, no host copy to wait for
// ---------------------------------------------------------------------------
constexpr int kEdgeChunk = 384;  // edges carried by one k_put_edges launch
struct EdgeChunk {
    double e[kEdgeChunk];
};

// static: one instance per translation unit that uploads edges, none of them exported
static __global__ void k_put_edges(double* __restrict__ dst, EdgeChunk c, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = c.e[threadIdx.x];
}

inline void put_edges(hipStream_t s, double* d_edges, const double* host_edges, int n) {
    for (int o = 0; o < n; o += kEdgeChunk) {
        EdgeChunk c;
        const int cnt = n - o < kEdgeChunk ? n - o : kEdgeChunk;
        memcpy(c.e, host_edges + o, sizeof(double) * cnt);
        hipLaunchKernelGGL(k_put_edges, dim3(1), dim3(kEdgeChunk), 0, s, d_edges + o, c, cnt);
    }
}

}  // namespace of3dk

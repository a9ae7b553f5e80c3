/*
 * of3d.h — C-ABI of the MI355X (gfx950) Lucas–Kanade optical-flow engine.
 *
 * Drop-in boundary for the hot path of ScientistRachel/OpticalFlow3D_dev:
 *   calc_flow3D(images, xyzSig, tSig, wSig) -> (vx, vy, vz, rel)   src/Python/calc_flow.py:175-360
 *   calc_flow2D(images, xySig,  tSig, wSig) -> (vx, vy, rel)       src/Python/calc_flow.py:18-173
 * The reference has no FFI of its own (pure NumPy/SciPy); the Python host in
 * opticalflow3d_dev_amd/calc_flow.py keeps those signatures and binds these
 * entry points with ctypes (binding shown in INTEGRATION.md).
 *
 * Conventions
 *  - Plain pointers and sizes only.  Arrays are C-ordered, x fastest:
 *    images (Nt, Nz, Ny, Nx) / (Nt, Ny, Nx); outputs (Nz, Ny, Nx) / (Ny, Nx).
 *  - Host entry points (of3d_flow3d / of3d_flow2d): the caller owns every host
 *    buffer; the library owns device memory (cached per shape+taps).
 *  - Device entry point (of3d_plan_execute): every pointer is device memory,
 *    work is enqueued on the given HIP stream (NULL = the device's null stream,
 *    HIP's own convention: ordered with the caller's default-stream work) and
 *    the call returns without synchronising.
 *  - Return 0 on success; non-zero = error, text in of3d_last_error()
 *    (thread-local).  The Python host maps the reference's argument checks
 *    (calc_flow.py:212-222) to SystemExit itself before calling in.
 *  - Taps are passed explicitly (full odd-length vectors, centre at index r),
 *    computed by the caller exactly as calc_flow.py:230-267 does; the library
 *    checks (anti)symmetry like scipy's NI_Correlate1D and uses the symmetric
 *    summation order (bit-exact with scipy.ndimage.correlate1d).
 */
#ifndef OF3D_H
#define OF3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OF3D_VERSION 10000 /* 1.0.0 */

/* element type of the input image stack (reference accepts any real dtype and
 * casts with images.astype(np.float64), calc_flow.py:225 / :67) */
enum of3d_dtype {
    OF3D_U8 = 1,
    OF3D_U16 = 2,
    OF3D_I16 = 3,
    OF3D_U32 = 4,
    OF3D_I32 = 5,
    OF3D_F32 = 6,
    OF3D_F64 = 7
};

/* arithmetic mode.  FP64_EXACT: fp64, no FMA contraction, scipy summation
 * order — vx/vy/vz bit-identical to the reference.  OR in OF3D_REL_F64 to get
 * the 3D reliability as float64 (the fp64 eigen-solve before the float32
 * cast; MATLAB's calc_flow3D.m:235-236 keeps rel in double).
 * OF3D_FP32 (plans only; configs[4]'s "fp32 path"): the filter passes and the
 * structure tensor in float32 (same scipy order), the 3x3 solve and the
 * eigenvalue in fp64, every output float32: half the workspace and HBM
 * traffic; accuracy max|dv| <= 1e-4 max|v| against the fp64 result. */
enum of3d_mode { OF3D_FP64_EXACT = 0, OF3D_REL_F64 = 0x100, OF3D_FP32 = 0x200 };

/* Filter taps (calc_flow.py:230-267).  Each vector has 2r+1 entries.
 * The reference's taps have rs <= rd (rs = ceil(3*sig/4)), and the tiled gradient kernels
 * stage an rd halo only.  Taps with rs > rd are accepted and run the general-radius path
 * (of3d_plan_kernels reports "general"): same arithmetic, no tuned kernels; a plane range's
 * input halo (of3d_plan_input_range) is then rw + max(rd, rs). */
typedef struct of3d_taps {
    const double* gauss;  /* fderiv == fx, radius rd = ceil(3*sig)       (:233,:253) */
    const double* deriv;  /* fderiv*gderiv, radius rd, antisymmetric     (:239)      */
    int rd;
    const double* smooth; /* fsmooth, radius rs = ceil(3*sig/4)          (:234)      */
    int rs;
    const double* tderiv; /* ft*gt, radius rt = ceil(3*tSig), antisym.    (:260)      */
    int rt;
    const double* window; /* gw, radius rw = ceil(3*wSig)                (:264)      */
    int rw;
} of3d_taps;

/* Optional timing record filled by the host entry points (milliseconds). */
typedef struct of3d_perf {
    double ms_h2d;     /* input upload                       */
    double ms_kernels; /* device time of the kernel pipeline  */
    double ms_d2h;     /* output download                     */
    double ms_total;   /* wall time of the call               */
} of3d_perf;

typedef struct of3d_plan of3d_plan;

/* Library version (OF3D_VERSION). */
int of3d_version(void);

/* Build provenance, a JSON object: {"src_hash": sha256 (first 16 hex digits) of the sources
 * the library was compiled from (csrc/Makefile HASH_FILES), "arch", "extra": the EXTRA
 * compile flags (empty for a product build), "flags"}.  The Python loader compares src_hash
 * with the sources beside the library and refuses a stale or EXTRA-flagged build.  No
 * reference counterpart (the reference has no compiled code). */
const char* of3d_build_info(void);

/* Last error message of the calling thread ("" if none). */
const char* of3d_last_error(void);

/* Number of visible HIP devices (0 when no GPU / no driver). */
int of3d_device_count(void);

/* Free the plans the host entry points cache (of3d_flow3d / of3d_flow2d keep the device
 * workspace of their last two shapes resident; tens of GB at configs[3]).  No reference
 * counterpart (calc_flow3D allocates per call). */
int of3d_cache_clear(void);

/* ---- host entry points (replace calc_flow3D / calc_flow2D) -------------- */

/* calc_flow3D (calc_flow.py:175-360).  images: (nt, nz, ny, nx) of `dtype`;
 * nt odd, only the centre frame c = (nt-1)/2 and frames c-rt..c+rt are read.
 * vx, vy, vz: float64 (nz, ny, nx); rel: float32 (nz, ny, nx) — the reference
 * returns rel from complex64 LAPACK, hence float32 (calc_flow.py:355-357) —
 * or float64 when mode has OF3D_REL_F64. */
int of3d_flow3d(const void* images, int dtype, int64_t nt, int64_t nz, int64_t ny, int64_t nx,
                const of3d_taps* taps, int mode, int device, double* vx, double* vy, double* vz,
                void* rel, of3d_perf* perf);

/* calc_flow2D (calc_flow.py:18-173).  images (nt, ny, nx); outputs float64
 * (ny, nx); rel = min root of the 2x2 characteristic quadratic (NaN where the
 * discriminant rounds negative, as NumPy gives). */
int of3d_flow2d(const void* images, int dtype, int64_t nt, int64_t ny, int64_t nx,
                const of3d_taps* taps, int mode, int device, double* vx, double* vy, double* rel,
                of3d_perf* perf);

/* ---- device-resident plan (streaming driver, benchmarks, z-slab shards) -- */

/* ndim 3: volume (nz, ny, nx); ndim 2: nz independent 2D frames processed
 * together (a batch of output frames: plane b of every frame pointer is the
 * image of window b, e.g. a series shifted by 0 .. 2rt frames; nz = 1 is
 * calc_flow2D's single frame).  Allocates the device workspace on `device`
 * for outputs over up to `max_out_planes` planes (<= 0: all nz). */
int of3d_plan_create(of3d_plan** plan, int ndim, int64_t nz, int64_t ny, int64_t nx,
                     const of3d_taps* taps, int mode, int device, int64_t max_out_planes);
int of3d_plan_destroy(of3d_plan* plan);

/* Device bytes held by the plan's workspace. */
size_t of3d_plan_workspace_bytes(const of3d_plan* plan);

/* Input planes a shard computing output planes [z_out0, z_out1) must hold
 * resident (global plane indices [*z_in0, *z_in1)): the stencil halo. */
int of3d_plan_input_range(const of3d_plan* plan, int64_t z_out0, int64_t z_out1, int64_t* z_in0,
                          int64_t* z_in1);

/* Run the pipeline for output planes [z_out0, z_out1) of the centre frame.
 * d_frames: host array of 2*rt+1 DEVICE pointers, frame c-rt .. c+rt of the
 *   stack, each pointing at global plane `frame_z0` of its frame (planes
 *   contiguous, row stride nx, plane stride ny*nx, elements of `dtype`).
 *   The frames must hold the planes of of3d_plan_input_range().
 * d_vx/d_vy/d_vz: float64 (z_out1-z_out0, ny, nx) (d_vz ignored for 2D);
 * d_rel: float32 for 3D (float64 if the plan's mode has OF3D_REL_F64),
 * float64 for 2D.  OF3D_FP32 plans: every output float32.
 * stream: hipStream_t, or NULL for the null stream (round 5; it used to mean the plan's own
 * non-blocking stream, which a torch caller passing its default stream's handle 0 got
 * unordered with its own kernels). */
int of3d_plan_execute(of3d_plan* plan, const void* const* d_frames, int dtype, int64_t frame_z0,
                      int64_t z_out0, int64_t z_out1, void* d_vx, void* d_vy, void* d_vz,
                      void* d_rel, void* stream);

/* Frame pipelining for a time series (the reference's per-frame loop, calc_flow.py:512-534):
 * of3d_plan_execute for d_frames, and — where the plan has the fused instance (uint16 frames,
 * serial schedule) — the W-z/solve kernel of this call also forms the temporal derivative of
 * the NEXT output frame from d_frames_next (2*rt+1 device pointers, same frame_z0 / planes;
 * their contents must be final when this call is enqueued).  The next of3d_plan_execute_next
 * call for exactly those frames and planes then skips its own K0 launch (a pure HBM stream
 * riding in the VALU-bound kernel's memory slack).  d_frames_next NULL: no lookahead.  Any
 * other call (of3d_plan_execute included) recomputes.  Results are bit-identical to
 * of3d_plan_execute (the same K0 arithmetic, k0_group). */
int of3d_plan_execute_next(of3d_plan* plan, const void* const* d_frames, const void* const* d_frames_next, int dtype,
                           int64_t frame_z0, int64_t z_out0, int64_t z_out1, void* d_vx, void* d_vy, void* d_vz,
                           void* d_rel, void* stream);

/* K0 batching for a time series (calc_flow.py:512-534 again): d_frames holds the frames
 * c-rt .. c+rt+n_ahead (2*rt+1+n_ahead device pointers: the current window, then the next
 * n_ahead frames, all resident and final when this call is enqueued).  of3d_plan_execute for
 * the window d_frames[0 .. 2rt]; where the plan runs the fused gradient kernel (serial
 * schedule, the vectorised frame layout) and no earlier call formed this window's temporal
 * derivative, one pass over the 2rt+1+m frames forms it AND the next m-1 windows' (m =
 * min(n_ahead, 4) + 1: 2rt+m frame reads for m derivatives instead of m(2rt+1)); the later
 * of3d_plan_execute_ahead calls for exactly those windows (frame pointers, dtype, frame_z0,
 * planes) skip their K0.  Calls on one stream (or otherwise ordered); any other execute call
 * drops the formed derivatives.  n_ahead past 65 - (2rt+1) frames is clamped (no batching
 * beyond the 65-frame pointer table); radii without a batched K0 instance (rt other than
 * 3, 6, 9) run the plain K0.  Bit-identical to of3d_plan_execute. */
int of3d_plan_execute_ahead(of3d_plan* plan, const void* const* d_frames, int n_ahead, int dtype, int64_t frame_z0,
                            int64_t z_out0, int64_t z_out1, void* d_vx, void* d_vy, void* d_vz, void* d_rel,
                            void* stream);

/* Per-stage timing with HIP events recorded on the launch stream.
 * of3d_plan_set_timing(plan, slots): keep a ring of `slots` executions
 * (0 = off; no host synchronisation is added to of3d_plan_execute).
 * of3d_plan_stage_times: average device time (ms) per stage over the
 * executions recorded since the previous read (at most `slots`), then reset;
 * returns the number of stages written (<= cap).  Stage names:
 * of3d_stage_name(i) = grad_xy, grad_z, prod_wy, wx, wz_solve.
 * of3d_plan_set_timing_mask(plan, mask): time only the stages in the bit
 * mask (bit i = stage i; default all).  Each event is a barrier packet
 * between two kernels, so fewer events perturb the pipeline less; stages
 * outside the mask read back as -1. */
int of3d_plan_set_timing(of3d_plan* plan, int slots);
int of3d_plan_set_timing_mask(of3d_plan* plan, unsigned mask);
int of3d_plan_stage_times(of3d_plan* plan, double* ms, int cap);

/* Overlap mode (3D plans with the fused products/W-xy kernel): of3d_plan_execute
 * splits the output planes into chunks of `chunk_planes` (<= 0: off, the default
 * unless OF3D_ZCHUNK is set; at most 16 chunks) and runs the HBM-bound gradient
 * stages of chunk c+1 on the caller's stream beside the VALU-bound W-xy / W-z /
 * solve stages of chunk c on the plan's second stream (joined back into the
 * caller's stream before the call's work completes).  Results are bit-identical
 * to the serial order.  A per-stage profile (timing mask with several stages)
 * runs serially; with one timed stage its time is summed over the chunks.  Fails while the
 * plan has an output row range (of3d_plan_set_rows), as set_rows fails on a chunked plan. */
int of3d_plan_set_overlap(of3d_plan* plan, int64_t chunk_planes);

/* Output rows (3D plans with the fused products/W-xy and W-z kernels): of3d_plan_execute
 * then writes only rows [y0, y1) of each output plane, as a compact (z_out1-z_out0,
 * y1-y0, nx) array; the earlier stages still run on every row (the W-y halo).  A row-slab
 * shard runs its rows + rd + rw halo rows as the plan's volume and keeps its own rows
 * this way (no reference counterpart: calc_flow.py:512's parallel loop, split by rows).
 * Fails (non-zero) where those kernels are not in use; (0, ny) restores the default. */
int of3d_plan_set_rows(of3d_plan* plan, int64_t y0, int64_t y1);

/* Kernel families this plan has launched so far, comma-separated (e.g.
 * "k_tderiv_c,k_grad_xyz_c,k_prod_wyx_ws,k_wz_solve_c"), written NUL-terminated into
 * buf (at most n bytes); returns the full length.  Diagnostics: which kernels a
 * parameter set / volume shape runs on (no reference counterpart). */
int of3d_plan_kernels(const of3d_plan* plan, char* buf, size_t n);
const char* of3d_stage_name(int i);

/* The plan's kernel geometry as a JSON object, written like of3d_plan_kernels (returns the
 * full length): the W-xy hand-off layout (wxy_zt: 0 plain planes, else z-tiled), the K34 shape
 * the autotune kept (staged columns, tile rows s, outputs per block, threads, candidates), the K5c
 * block (planes per z-group, waves), and of the LAST execution the K12 march length and grid and
 * the batched-K0 windows.  "runtime_radius": the template instances the runtime-radius kernels'
 * getters pick for the plan's radii (k1_nj: k_grad_xy rows per thread; k3_tj, k4_tj: k_prod_wy /
 * k_wx; k5 {r, nj}: k_wz_solve planes per thread and window rows per thread; k5_dma {nb, nj2}:
 * k_wz_solve_dma window buffers, 0 where the register-staged k_wz_solve runs, and row groups
 * per wave; general: the general-radius path runs instead, the others are 0).
 * Diagnostics for tests and benchmarks (no reference counterpart). */
int of3d_plan_geometry(const of3d_plan* plan, char* buf, size_t n);

/* Copy `bytes` from src to dst on `stream` with a kernel of at most
 * `max_blocks` workgroups (0 = 64).  Either side may be pinned host memory
 * (hipHostMalloc / torch pin_memory): used to download a frame's outputs
 * over PCIe while the next frame's kernels keep the rest of the GPU (the
 * runtime's own device->host copy runs as a full-GPU blit kernel).
 * No reference counterpart: process_flow's per-frame output transfer
 * (calc_flow.py:526-529 writes host arrays). */
int of3d_copy_async(void* dst, const void* src, size_t bytes, int max_blocks, void* stream);

/* Downstream statistics on resident outputs (device pointers), one pass —
 * the reference's example_analysis_script.ipynb cells 4-6:
 * mask = rel > thresh (thresh: e.g. the 90th percentile of rel); each of
 * vx, vy, vz multiplied by the mask, exact zeros -> NaN, then scaled to
 * physical units ((v*xyscale)/tscale; vz with zscale); magnitude, theta =
 * atan2(vy, vx), phi = atan(vz / sqrt(vx^2 + vy^2)).  Inputs float64 (or
 * float32 with v_f32), rel float32 (or float64 with rel_f64); outputs
 * float64.  2D: vz = out_vz = phi = NULL.  Enqueued on `stream`. */
int of3d_flow_stats(const void* vx, const void* vy, const void* vz, const void* rel, int v_f32, int rel_f64,
                    int64_t n, double thresh, double xyscale, double zscale, double tscale, double* out_vx,
                    double* out_vy, double* out_vz, double* magnitude, double* theta, double* phi, void* stream);

/* Exact order statistics of a device array without leaving the device (radix select on the
 * order-preserving integer image of the float bits, 11-bit digits: 3 passes over float32, 6
 * over float64): the element of 0-based rank `lo` (a) and of rank `hi` (b) of the n values
 * (float32, or float64 with is_f64), lo <= hi <= n-1, combined as numpy's 'linear'
 * percentile does in the array's dtype: a + (b-a)*gamma for gamma < 0.5, else
 * b - (b-a)*(1-gamma); a when lo == hi (by the same expression, so an infinite a gives NaN as
 * numpy's does); NaN when the array holds a NaN.  -0.0 and +0.0 are one value.  `out`: one device element of the array's dtype.  Everything is enqueued on
 * `stream`; nothing is copied to the host and nothing synchronises, so the value can feed the
 * next kernel (of3d_flow_summary's d_thresh).  `workspace`: device memory of
 * of3d_quantile_workspace_bytes(is_f64) bytes (independent of n), 8-byte aligned.
 * The reference takes np.percentile(rel, relPer) on the host (example_analysis_script.ipynb
 * cell 4). */
size_t of3d_quantile_workspace_bytes(int is_f64);
int of3d_quantile(const void* d_a, int is_f64, int64_t n, int64_t lo, int64_t hi, double gamma, void* d_out,
                  void* workspace, void* stream);

/* Frame summary on resident outputs: of3d_flow_stats' per-voxel arithmetic (mask = rel >
 * *d_thresh, a threshold in rel's dtype on the device; v*mask, exact zeros -> NaN,
 * (v*scale)/tscale; magnitude; theta = atan2(vy, vx); phi = atan(vz / sqrt(vx^2+vy^2)), 3D
 * only) reduced over n_roi <= 16 boxes of the (nz, ny, nx) volume instead of stored: what the
 * reference's figure scripts compute from the saved TIFFs (plot_figure4_timeTraces.m:82-126,
 * plot_figure3_ROIfigures.m:114-193).  rois: host int64[n_roi][6] = z0 z1 y0 y1 x0 x1,
 * half-open, inside the volume and not empty.  A voxel is valid when its magnitude is not NaN.
 * nbins: host int[6], edges: host double*[6] (entry q: nbins[q] + 1 strictly ascending edges;
 * ignored where nbins[q] == 0) for the quantities 0 vx, 1 vy, 2 vz, 3 magnitude, 4 theta,
 * 5 phi; at most 256 bins each, 0 = no histogram; np.histogram(values, bins=edges) semantics
 * over the valid voxels (last bin closed, values outside and NaN dropped; counts —
 * of3d_flow_whist gives the magnitude-weighted ones).  2D: vz == NULL, nz == 1, nbins[2] == nbins[5] == 0.
 *
 * Result (device, of3d_flow_summary_result_bytes(n_roi, nbins) bytes, 8-byte words):
 *   word 0        the threshold as float64
 *   word 1        n_roi (uint64)
 *   words 2..7    nbins[0..5] (uint64)
 *   then per box, 10 + sum(nbins) words:
 *     0  n_valid (int64)      1  n_voxels (int64)
 *     2..9  float64 sums over the valid voxels: magnitude, vx, vy, vz (0 in 2D), sin(theta),
 *           cos(theta), magnitude*sin(theta), magnitude*cos(theta)  (sin = vy/h, cos = vx/h,
 *           h = sqrt(vx^2+vy^2))
 *     10..  uint64 histogram counts, quantity after quantity (nbins[q] words each)
 * Deterministic: no floating-point atomics; the workgroups of a box are a function of the
 * box's size alone, each sums in a fixed order into its own workspace slot, and a second
 * kernel adds the slots in index order, so equal inputs give equal bits on every run and a
 * box's words do not depend on the other boxes.  `workspace`: device memory of
 * of3d_flow_summary_workspace_bytes() bytes.  Enqueued on `stream`; no host synchronisation. */
#define OF3D_SUMMARY_QUANTITIES 6
#define OF3D_SUMMARY_MAX_BINS 256
#define OF3D_SUMMARY_MAX_ROI 16
size_t of3d_flow_summary_result_bytes(int n_roi, const int* nbins);
size_t of3d_flow_summary_workspace_bytes(void);
int of3d_flow_summary(const void* d_vx, const void* d_vy, const void* d_vz, const void* d_rel, int v_f32,
                      int rel_f64, int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale,
                      double zscale, double tscale, const int64_t* rois, int n_roi, const int* nbins,
                      const double* const* edges, void* d_result, void* workspace, void* stream);

/* Area opening of the reliability mask on the device: MATLAB's
 *   relMask = rel > relThresh;  relMask = bwareaopen(relMask, minSize);
 * of the reference's figure scripts (plot_figure4_timeTraces.m:75-79, plot_figure4_Movies.m:93-94,
 * plot_figure5.m:87-88, plot_figure5_Movie.m:88-89; plot_figure3_ROIfigures.m:96 and
 * plot_figure3_ChannelCompare.m:140 with 10^5), applied to each cropped ROI as
 * plot_figure4_timeTraces.m:72-79 does.  d_rel: (nz, ny, nx) float32 (float64 with rel_f64),
 * 2D = nz 1; d_thresh: one device element of rel's dtype (of3d_quantile's output); rois as
 * of3d_flow_summary's; min_size >= 1; connectivity 6, 18 or 26 for nz > 1, 4 or 8 for nz == 1
 * (bwareaopen's defaults are 26 and 8).  For every box r independently:
 *   1. M_r = (rel > *d_thresh) restricted to the box (a NaN on either side gives false);
 *   2. the connected components of M_r inside the box (neighbours outside it connect nothing);
 *   3. keep_r = the union of the components with at least min_size voxels.
 * d_keep: one uint16 per voxel of the whole volume; bit r is set where the voxel lies in box r
 * and in keep_r, every other bit is 0 (boxes may overlap, a voxel's bits may differ).
 * d_counts: int64[n_roi][4] = n_mask (voxels of M_r), n_components, n_components_kept, n_kept
 * (voxels of keep_r).  min_size 1 keeps every mask voxel.
 * Union-find over box-local uint32 labels, one launch per phase and box (initial labels with
 * the x-runs of a wave pre-merged, unions with the backward neighbours by find + atomicMin,
 * path compression, component sizes by integer atomics, the keep bits): every component is
 * rooted at its smallest linear index, so all outputs are integers fixed by the input alone —
 * equal bits on every run and exactly a host labelling's result.  A box needs fewer than
 * 2^32 - 1 voxels.  `workspace`: device memory of of3d_mask_open_workspace_bytes(rois, n_roi)
 * bytes (labels and sizes of the largest box, 8 bytes per voxel; 0 for invalid boxes), shared
 * by the boxes.  Enqueued on `stream`; no host synchronisation, no workgroup waits for another. */
size_t of3d_mask_open_workspace_bytes(const int64_t* rois, int n_roi);
int of3d_mask_open(const void* d_rel, int rel_f64, int64_t nz, int64_t ny, int64_t nx, const void* d_thresh,
                   const int64_t* rois, int n_roi, int64_t min_size, int connectivity, uint16_t* d_keep,
                   int64_t* d_counts, void* workspace, void* stream);

/* The largest connected component of the reliability mask on the device: what the reference's
 * plot_figure2_movie.ipynb cell 1 does with
 *   labels_mask = measure.label(relMask); regions.sort(key=lambda x: x.area, reverse=True)
 * and zeroing every region but the first ("some cells have a small piece of another cell in the
 * FOV").  Arguments, M_r, its components and the connectivities are of3d_mask_open's (26 and 8 are
 * measure.label's full connectivity); there is no min_size, because the sizes are not known
 * beforehand.  For every box r independently keep_r is the one component of M_r with the most
 * voxels; among components of equal size the one with the smallest root, i.e. the one that holds
 * the smallest linear index of the box — the lowest label of a raster-order labelling, which is
 * what the script's stable sort keeps.  An empty M_r keeps nothing.
 * d_keep and d_counts have of3d_mask_open's layout: bit r of one uint16 per voxel (cleared on the
 * stream first), int64[n_roi][4] = n_mask, n_components, n_components_kept (0 or 1), n_kept; so
 * d_keep feeds of3d_flow_summary_masked, of3d_mask_axes, of3d_flow_whist, of3d_quiver_sample and
 * of3d_flow_contract unchanged.
 * The init, merge and count phases are of3d_mask_open's kernels.  Then every root offers the key
 * (size << 32) | (0xFFFFFFFF - root) to one 64-bit word of the box by an integer atomicMax — the
 * maximum does not depend on the order of the offers — and a last phase sets bit r where the
 * voxel's label is the winner.  A box has fewer than 2^32 - 1 voxels, so a size fits the key's
 * upper half.  `workspace`: of3d_mask_largest_workspace_bytes(rois, n_roi) bytes — of3d_mask_open's
 * plus one word per box; 0 for invalid boxes.  Enqueued on `stream`; no host synchronisation, no
 * workgroup waits for another. */
size_t of3d_mask_largest_workspace_bytes(const int64_t* rois, int n_roi);
int of3d_mask_largest(const void* d_rel, int rel_f64, int64_t nz, int64_t ny, int64_t nx, const void* d_thresh,
                      const int64_t* rois, int n_roi, int connectivity, uint16_t* d_keep, int64_t* d_counts,
                      void* workspace, void* stream);

/* of3d_flow_summary with the mask factor of a voxel in box r taken from bit r of d_keep
 * (of3d_mask_open's output) instead of rel > *d_thresh: the figure scripts' statistics over the
 * opened mask.  Word 0 of the result is still *d_thresh; the result layout, the workgroup
 * partition, the summation order and the histograms are of3d_flow_summary's, so a d_keep from
 * min_size 1 gives of3d_flow_summary's bits. */
int of3d_flow_summary_masked(const void* d_vx, const void* d_vy, const void* d_vz, const void* d_rel, int v_f32,
                             int rel_f64, int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale,
                             double zscale, double tscale, const int64_t* rois, int n_roi, const int* nbins,
                             const double* const* edges, void* d_result, void* workspace, void* stream,
                             const uint16_t* d_keep);

/* The body-axis frame of the reliability mask and the flow projected onto it, on the device:
 * what the reference's plot_figure5.m:87-88,132-149,200 and plot_figure5_Movie.m:88-89,128-143 do
 * with regionprops3(relMask, 'EigenVectors', 'EigenValues') and a projection of every physical
 * velocity vector onto the first eigenvectors (the embryo's anterior-posterior and dorso-ventral
 * axes).  Fields, d_rel, dtypes, dims, d_thresh, scales and rois as of3d_flow_summary's.  For
 * every box r independently:
 *   1. the mask M_r: bit r of d_keep (of3d_mask_open's output) when d_keep is given, else
 *      rel > *d_thresh inside the box (a NaN gives false; d_rel / d_thresh may be NULL with
 *      d_keep).  A NaN magnitude plays no part here: regionprops3 sees only the mask.
 *   2. ten unsigned 64-bit sums over M_r of the box-local integer coordinates (x - x0, y - y0,
 *      z - z0): n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz.  Integer arithmetic and integer
 *      atomics only: exact and independent of the order.
 *   3. centroid = box origin + S_a / n, in volume coordinates (x, y, z); the population
 *      covariance C_ab = (n S_ab - S_a S_b) / n^2, the numerator exact in 128-bit integers,
 *      converted to float64 as hi * 2^64 + lo, then divided by (double)n * (double)n; with
 *      axes_physical C becomes S C S, S = diag(xyscale, xyscale, zscale).
 *   4. eigenvalues (descending, as regionprops3 lists them; one that rounding left negative is
 *      0) and unit eigenvectors of C by a cyclic Jacobi iteration in float64 (12 sweeps, no
 *      data-dependent loop); equal eigenvalues keep the x, y, z order.  Sign: the component of
 *      largest magnitude of each vector is positive, a tie goes to the first of x, y, z.  A 2D
 *      volume (nz == 1) gives eigenvalue 3 = 0 and vector 3 = (0, 0, 1).  n == 0: NaN.
 *   5. the axes used: the box's eigenvectors e1 e2 e3, or axes_given (host, 9 finite doubles
 *      e1 e2 e3, each x y z, the same for every box; they travel as kernel arguments) — a
 *      movie keeps one frame's axes so that no sign flips between frames.  Steps 2-4 are
 *      reported either way.
 *   6. with fields (d_vx != NULL): of3d_flow_summary's per-voxel arithmetic (mask factor,
 *      v * mask, zeros -> NaN, (v*scale)/tscale; valid <=> magnitude not NaN), then
 *      p_k = (vx*e_k.x + vy*e_k.y) + vz*e_k.z (2D: vx*e_k.x + vy*e_k.y), plain multiplies and
 *      adds in that order (no FMA); n_valid, the three sums of p_k and up to three histograms
 *      (nbins3: host int[3], edges3: host double*[3]; np.histogram semantics, at most 256 bins;
 *      nbins3[2] == 0 in 2D).  d_vx == NULL (then d_vy == d_vz == NULL, nbins3 all 0): steps
 *      1-5 only.
 * Not reproduced of regionprops3: any constant it adds to the second moments for a voxel's own
 * extent (a multiple of the identity: the eigenvectors are the same, the eigenvalues shift by
 * it), and the scripts' pairing vy*vecs(1,k) + vx*vecs(2,k): here the x component of an axis
 * multiplies vx; the axes are returned, so any other pairing can be formed from them.
 *
 * Result (device, of3d_mask_axes_result_bytes(n_roi, nbins3) bytes, 8-byte words), per box
 * 44 + sum(nbins3) words:
 *    0..9    uint64 n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz
 *   10..12   float64 centroid x y z
 *   13..18   float64 covariance xx yy zz xy xz yz
 *   19..21   float64 eigenvalues, descending
 *   22..30   float64 eigenvectors e1 e2 e3, each x y z
 *   31..39   float64 the axes used for the projection, e1 e2 e3
 *   40       n_valid (int64)
 *   41..43   float64 sums of p_1, p_2, p_3 over the valid voxels (p_3: vz term omitted in 2D)
 *   44..     uint64 histogram counts, axis after axis (nbins3[k] words each)
 * Deterministic as of3d_flow_summary is (the same workgroup partition, summation order and
 * slots; no floating-point atomics), and a box's words do not depend on the other boxes.
 * of3d_mask_axes_workspace_bytes: host arithmetic only; 0 for an invalid box and for a box whose
 * sums could overflow: voxels * (L - 1)^2 < 2^63 is required, L the box's longest edge.
 * Enqueued on `stream`; no host synchronisation, no workgroup waits for another. */
#define OF3D_AXES_QUANTITIES 3
#define OF3D_AXES_ROI_WORDS 44
size_t of3d_mask_axes_workspace_bytes(const int64_t* rois, int n_roi);
size_t of3d_mask_axes_result_bytes(int n_roi, const int* nbins3);
int of3d_mask_axes(const void* d_vx, const void* d_vy, const void* d_vz, const void* d_rel, int v_f32, int rel_f64,
                   int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                   double tscale, const int64_t* rois, int n_roi, const uint16_t* d_keep, const double* axes_given,
                   int axes_physical, const int* nbins3, const double* const* edges3, void* d_result,
                   void* workspace, void* stream);

/* Magnitude-weighted histograms of the frame summary: per box and quantity
 *   np.histogram(values, bins=edges, weights=magnitude)[0]
 * over the valid voxels — the reference's distPhiW (plot_figure4_timeTraces.m:128-138:
 * accumarray(discretize(-phi, phiBins), mag) over ~badRows; its division by the valid count is
 * left to the caller, n_valid is returned).  Fields, d_rel, dtypes, dims, d_thresh, scales, rois,
 * validity (magnitude not NaN), nbins, edges and the bin rule are of3d_flow_summary's; the weight
 * is always the physical magnitude.  d_keep NULL: the mask factor is rel > *d_thresh; else bit r
 * of d_keep for box r, as of3d_flow_summary_masked (d_rel and d_thresh may then be NULL).  At
 * least one quantity must have bins; 2D: vz == NULL, nz == 1, nbins[2] == nbins[5] == 0.
 *
 * Result (device, of3d_flow_whist_result_bytes(n_roi, nbins) bytes, 8-byte words, zeroed on the
 * stream first), per box 1 + sum(nbins) words:
 *   0    n_valid (int64; of3d_flow_summary's for the same mask)
 *   1..  float64 bin sums, requested quantity after quantity in the order vx, vy, vz, magnitude,
 *        theta, phi (nbins[q] words each)
 * A pass over the fields per requested quantity (grid: workgroups x boxes x quantities), beside
 * of3d_flow_summary's and with its workgroup partition.  Deterministic under the same contract:
 * no floating-point atomic in LDS or global memory.  Every wave keeps a bin array of its own in
 * LDS; per voxel step it visits the distinct bins among its 64 lanes in the order of their first
 * lane, adds the weights of the lanes holding the bin (+0.0 in the others, exact as weights are
 * >= 0) by a fixed shuffle tree and one lane adds that to the wave's array; the workgroup adds
 * its waves' arrays in wave order into its own workspace slot, and a second kernel adds a bin's
 * slots in workgroup order.  Each bin's summation order is fixed by the box, the thread, wave and
 * slot indices and the data, so equal inputs give equal bits on every run, and a box's words
 * depend neither on the other boxes nor on which other quantities are requested.
 * `workspace`: device memory of of3d_flow_whist_workspace_bytes(rois, n_roi, nbins) bytes — the
 * edges, then one slot of sum(nbins) float64 per workgroup of every box; host arithmetic only,
 * 0 (and of3d_last_error's text) for an invalid box or no bins.  Enqueued on `stream`; no host
 * copy, no host synchronisation, no workgroup waits for another. */
size_t of3d_flow_whist_result_bytes(int n_roi, const int* nbins);
size_t of3d_flow_whist_workspace_bytes(const int64_t* rois, int n_roi, const int* nbins);
int of3d_flow_whist(const void* d_vx, const void* d_vy, const void* d_vz, const void* d_rel, int v_f32, int rel_f64,
                    int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                    double tscale, const int64_t* rois, int n_roi, const uint16_t* d_keep, const int* nbins,
                    const double* const* edges, void* d_result, void* workspace, void* stream);

/* Area opening of the JOINT reliability mask of two channels (figure 3: myosin and actin):
 *   relMask = (rel > prctile(rel(:),relPer)) | (rel1 > prctile(rel1(:),relPer));
 *   relMask = relMask & (rel > 0) & (rel1 > 0);   relMask = bwareaopen(relMask, 10^5);
 * (plot_figure3_ROIfigures.m:93-96, plot_figure3_ChannelCompare.m:137-140: one mask for both
 * channels, "for a fair comparison of dot products, magnitude, etc.").  d_rel0, d_rel1: two
 * fields of one dtype (rel_f64) and shape; d_thresh0, d_thresh1: one device element each of that
 * dtype (of3d_quantile's output per channel).  For every box r the mask is
 *   M_r = C(rel0 > *t0, rel1 > *t1) && ((double)rel0 > floor) && ((double)rel1 > floor)
 * cropped to the box; C is OR for combine == 0 (the scripts'), AND for combine == 1, anything
 * else is an error.  A NaN field value gives false (it fails the floor clause whatever the
 * floor); a NaN threshold makes its own comparison false everywhere, so that under OR the other
 * channel decides and under AND nothing passes.  The scripts' floor is 0; -INFINITY switches the
 * clause off (only NaN and -inf then fail it); a NaN floor is an error.
 * Everything after the predicate is of3d_mask_open's, by the same kernels: the components inside
 * the box, min_size >= 1, connectivity 4 / 8 or 6 / 18 / 26, bit r of d_keep, d_counts[n_roi][4],
 * the workspace of of3d_mask_open_workspace_bytes(rois, n_roi), stream ordering, no host
 * synchronisation, no workgroup waiting for another.  d_keep has of3d_mask_open's format, so it
 * also feeds of3d_flow_pair, of3d_mask_axes, of3d_flow_summary_masked and of3d_flow_whist.
 * rel1 == rel0 with equal thresholds and floor -INFINITY gives of3d_mask_open's bits. */
int of3d_mask_open_pair(const void* d_rel0, const void* d_thresh0, const void* d_rel1, const void* d_thresh1,
                        int rel_f64, double floor, int combine, int64_t nz, int64_t ny, int64_t nx,
                        const int64_t* rois, int n_roi, int64_t min_size, int connectivity, uint16_t* d_keep,
                        int64_t* d_counts, void* workspace, void* stream);

/* Two channels' flows of one frame compared over the same voxels, in one pass over both
 * channels' fields: what the reference's figure 3 reduces them to
 * (plot_figure3_ROIfigures.m:98-193, plot_figure3_ChannelCompare.m:142-164: the velocities under
 * the joint mask, theta / theta1, mag / mag1, badRows = isnan(theta) | isnan(theta1), then per
 * ROI the plain and magnitude-weighted circular means of both channels over ~badRows), with the
 * per-voxel comparisons the scripts' joint mask is made for.  d_vx0.. / d_vx1..: the channels'
 * fields, one dtype (v_f32), shape and set of scales (one acquisition); d_vz0 and d_vz1 both
 * given, or both NULL: the in-plane mode, legal for any nz (figure 3 uses the in-plane magnitude
 * and theta of a 3-slice volume).  d_keep (required): of3d_mask_open_pair's output, or any other
 * keep volume; min_size 1 there gives the unopened mask.  rois as of3d_flow_summary's.
 * Per voxel of box r, m = bit r of d_keep as 1.0 / 0.0:
 *   every component of both channels: v*m, an exact zero -> NaN, (v*scale)/tscale;
 *   mag_c = sqrt(vx^2 + vy^2 [+ vz^2]) in of3d_flow_summary's expression order;
 *   valid <=> mag_0 and mag_1 are both not NaN (in-plane: ~(isnan(theta) | isnan(theta1)));
 *   h_c = sqrt(vx_c^2 + vy_c^2), sn_c = vy_c/h_c, cs_c = vx_c/h_c;
 *   dot = (vx0*vx1 + vy0*vy1) + vz0*vz1 (in-plane: without the z term);
 *   cosine = dot / (mag0*mag1) — NOT clamped: rounding may leave it a few ulp beyond +-1, and
 *     such a value falls outside histogram edges that end at +-1 (end the edges a little wider);
 *   cosD = cs0*cs1 + sn0*sn1, sinD = cs0*sn1 - sn0*cs1, dtheta = atan2(sinD, cosD) (histogram only);
 *   diff = sqrt(((vx1-vx0)^2 + (vy1-vy0)^2) + (vz1-vz0)^2);  dmagnitude = mag1 - mag0;
 * plain multiplies and adds in the written order (no FMA).
 *
 * Result (device, of3d_flow_pair_result_bytes(n_roi, nbins4) bytes, 8-byte words, zeroed on the
 * stream first), per box OF3D_PAIR_ROI_WORDS + sum(nbins4) words:
 *    0       n_valid (int64)         1  n_voxels (int64)
 *    2..9    channel 0: of3d_flow_summary's eight float64 sums over the valid voxels (magnitude,
 *            vx, vy, vz [0 in-plane], sin(theta), cos(theta), magnitude*sin, magnitude*cos)
 *   10..17   channel 1: the same
 *   18..25   float64 sums of dot, cosine, mag0*mag1, mag0^2, mag1^2, sinD, cosD, diff
 *   26..     uint64 histogram counts of dot, cosine, dtheta, dmagnitude (nbins4[q] words each;
 *            np.histogram semantics, at most 256 bins, edges4: host double*[4]; all 0 is legal)
 * atan2(sum sin, sum cos) and atan2(sum mag*sin, sum mag*cos) of a channel's block are the
 * scripts' ch0_theta / ch0_thetaW (atan2 is invariant under the common positive factor 1/n).
 * Deterministic under of3d_flow_summary's contract: its workgroup partition, per-thread
 * accumulators in a fixed order, a fixed shuffle tree over the lanes, the waves' partials in wave
 * order into the workgroup's own workspace slot, a second kernel adding a sum's slots in
 * workgroup-index order; counts by integer atomics; no floating-point atomic.  Equal inputs give
 * equal bits on every run, a box's words do not depend on the other boxes, and where every kept
 * voxel is valid in both channels a channel's block is bitwise of3d_flow_summary_masked's for the
 * same d_keep.
 * `workspace`: device memory of of3d_flow_pair_workspace_bytes(rois, n_roi, nbins4) bytes — the
 * edges, then one slot of 24 float64 per workgroup of every box; host arithmetic only, 0 (and
 * of3d_last_error's text) for an invalid box, more than 16 boxes or a workgroup share of 2^31
 * voxels or more.  Enqueued on `stream`; no host copy, no host synchronisation, no workgroup
 * waits for another. */
#define OF3D_PAIR_QUANTITIES 4 /* histograms: 0 dot, 1 cosine, 2 dtheta, 3 dmagnitude */
#define OF3D_PAIR_ROI_WORDS 26
size_t of3d_flow_pair_result_bytes(int n_roi, const int* nbins4);
size_t of3d_flow_pair_workspace_bytes(const int64_t* rois, int n_roi, const int* nbins4);
int of3d_flow_pair(const void* d_vx0, const void* d_vy0, const void* d_vz0, const void* d_vx1, const void* d_vy1,
                   const void* d_vz1, int v_f32, int64_t nz, int64_t ny, int64_t nx, double xyscale, double zscale,
                   double tscale, const int64_t* rois, int n_roi, const uint16_t* d_keep, const int* nbins4,
                   const double* const* edges4, void* d_result, void* workspace, void* stream);

/* Quiver samples of the frame summary: per box the vectors that the reference's figure scripts
 * hand to quiver / quiver3 — every gap-th voxel of the ROI whose masked velocity is not NaN
 * (example_analysis_script.m:64-66,121-135, plot_figure4_Movies.m:121-143, plot_figure5.m:119-156,
 * plot_FigureS2_dt.m:99-143, plot_figure3_ChannelCompare.m:181) — as an ordered list, so that a
 * summary-only series (no field downloads) can still be drawn.  Fields, d_rel, dtypes, dims,
 * d_thresh, scales and rois as of3d_flow_summary's; d_keep NULL: the mask factor is
 * rel > *d_thresh, else bit r of d_keep for box r, as of3d_flow_summary_masked (d_rel and d_thresh
 * may then be NULL; word 0 of the result is NaN without a d_thresh).  gap3: host int64[3] =
 * gz gy gx, each >= 1.  capacity: host int64[n_roi], each >= 0.  For every box r independently:
 *   lattice  the voxels (z0 + i*gz, y0 + j*gy, x0 + k*gx) inside the box — anchored at the box
 *            origin, as y1:gap:y2 is in the scripts; n_lattice of them;
 *   valid    of3d_flow_summary's predicate: every component v * mask factor, an exact zero ->
 *            NaN, (v*scale)/tscale (vz with zscale); valid <=> the magnitude is not NaN;
 *   output   the valid lattice voxels in C order (z, then y, then x ascending): the voxel's
 *            linear index in the whole volume and its three physical velocities as float64 (vz 0.0
 *            in 2D) — for a numpy user f[z0:z1:gz, y0:y1:gy, x0:x1:gx][valid] of each field;
 *   capacity n_valid is always the full count, n_stored = min(n_valid, capacity[r]), the stored
 *            records are the first n_stored in that order; nothing is written past the block.
 * 2D: d_vz == NULL and nz == 1 (a d_vz with nz == 1 is an error).
 *
 * Result (device, of3d_quiver_result_bytes(n_roi, capacity) bytes, 8-byte words):
 *   word 0        the threshold as float64
 *   words 1..5    n_roi, gz, gy, gx, has_vz (int64)
 *   then per box, 4 words: n_lattice, n_valid, n_stored, the word offset of the box's block
 *   then per box its block, 4 * capacity[r] words: capacity[r] linear indices (int64), then as
 *   many vx, vy and vz (float64).  The words of an array past n_stored are unspecified.
 * Three launches on `stream`: (1) per box sum_workgroups(lattice points, lattice rows) workgroups
 * — a function of the box and the gap alone —, each over a contiguous run of lattice rows, split
 * into one contiguous sub-run per wave; a wave walks its sub-run 64 consecutive lattice points
 * per step and adds up the population count of the 64-bit ballot of `valid`; one count per wave
 * goes to the workspace.  (2) One workgroup per box scans the wave counts (exclusive, in
 * workgroup-then-wave order = C order) and writes the header.  (3) The walk of (1) again, by the
 * same device function: a lane's record index is its wave's base + the valid lanes below it;
 * records below the capacity are stored by plain stores.  No atomics of any kind: a record's
 * place and value are fixed by the inputs alone, so equal inputs give equal bits on every run,
 * and a box's counts and records do not depend on the other boxes.
 * `workspace`: device memory of of3d_quiver_workspace_bytes(rois, n_roi, gap3) bytes, one word per
 * wave of every workgroup; host arithmetic only.  Both *_bytes functions return 0 (and
 * of3d_last_error's text) on a refusal: a null pointer, an invalid box, more than 16 boxes, a gap
 * below 1, a negative capacity, a workgroup share of 2^31 lattice points or more.  Enqueued on
 * `stream`; no host copy, no host synchronisation, no workgroup waits for another. */
#define OF3D_QUIVER_HEAD_WORDS 6
#define OF3D_QUIVER_ROI_WORDS 4
size_t of3d_quiver_result_bytes(int n_roi, const int64_t* capacity);
size_t of3d_quiver_workspace_bytes(const int64_t* rois, int n_roi, const int64_t* gap3);
int of3d_quiver_sample(const void* d_vx, const void* d_vy, const void* d_vz, const void* d_rel, int v_f32, int rel_f64,
                       int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                       double tscale, const int64_t* rois, int n_roi, const int64_t* gap3, const int64_t* capacity,
                       const uint16_t* d_keep /* NULL: rel > *d_thresh */, void* d_result, void* workspace,
                       void* stream);

/* Field export: the fields themselves, cropped to the boxes of the frame summary, masked the way
 * the reference's scripts mask them right after loading them, in physical units, optionally
 * narrowed to float32, as compact blocks — what every figure script keeps of the four full-size
 * outputs (vx(y1:y2,x1:x2,z1:z2), then vx.*relMask./relMask*xyscale/tscale in plot_figure3 / 4 / 5,
 * vx.*relMask in plot_FigureS2_dt.m:123, vx*relMask; vx[vx==0]=nan in the notebooks), so that the
 * download, the pinned memory and the files scale with the ROI instead of the volume.  Fields,
 * d_rel, dtypes, dims, d_thresh, scales and rois as of3d_flow_summary's; d_keep as
 * of3d_quiver_sample's (NULL: the mask factor is rel > *d_thresh, else bit r of d_keep for box r).
 * Only what the call uses must be given: the requested fields, and with a mask_mode other than 0
 * d_keep, or d_rel and d_thresh.  2D: d_vz == NULL and nz == 1 (a d_vz with nz == 1, and the vz bit
 * without a d_vz, are errors).
 * fields: bit 0 vx, 1 vy, 2 vz, 3 rel: the fields exported, one at least.  Bit
 * OF3D_EXPORT_SKIP_SHIFT + r: box r is listed but not exported — it keeps its index, and so its bit
 * of d_keep, and has no blocks (the boxes of a summary of which only some are wanted).
 * Per voxel of box r, with m the mask factor as 0.0 or 1.0 and s = xyscale (zscale for vz):
 *   mask_mode 0 (none)     v                                    the plain crop
 *             1 (nan)      (v * m) / m                          v.*relMask./relMask
 *             2 (zero)     v * m                                v.*relMask
 *             3 (summary)  v * m, then an exact zero -> NaN     of3d_flow_summary's masking
 *   physical               then (x * s) / tscale, in that order
 * every operation an fp64 operation of its own (a float32 v is widened first; no FMA contraction),
 * so -3.0 * 0.0 is -0.0 and inf * 0.0 is NaN.  rel is always the plain crop.  out_f32 narrows every
 * finished float64 value with one round-to-nearest conversion; without it a field keeps its own
 * type (a float32 field's values are computed in fp64 and rounded once).  A value that no
 * arithmetic and no conversion touches (mode 0 without physical in the field's own type; rel in its
 * own type) is a bit copy, NaN payloads and -0.0 included.
 *
 * Result (device, of3d_field_export_result_bytes(...) bytes, 8-byte words; d_result 16-byte aligned):
 *   word 0        the threshold as float64 (NaN without a d_thresh)
 *   words 1..7    n_roi, fields, mask_mode, physical, out_f32, has_vz, the total word count (int64)
 *   then per box, 6 words: its voxel count, the element sizes (velocity blocks' + 256 * the rel
 *   block's, in bytes), the word offsets of its vx, vy, vz and rel blocks (0: not exported)
 *   then the blocks, box by box and vx, vy, vz, rel within a box: each starts on a 16-byte
 *   boundary, holds the box's dz * dy * dx elements in C order and is padded to whole 16 bytes
 *   with zeros.
 * Every byte of the result is written by the call, and nothing outside it.  One launch on `stream`
 * for all blocks, and a one-workgroup launch behind it for the header.  The blocks' launch has the
 * grid (workgroups, box, field); box r has sum_workgroups(voxels, rows) workgroups — a function of
 * the box alone — over contiguous runs of 16-byte groups of a block; a lane owns one group (2 fp64
 * or 4 fp32 consecutive elements of the compact block) per step and stores it with one aligned
 * 16-byte store whatever x0 and dx are; a group may straddle a row end of the box, the source
 * address is formed per element.  Every output element has one writer: no atomics, no workspace,
 * no host copy, no host synchronisation, no workgroup waits for another.
 * of3d_field_export_result_bytes: host arithmetic only; 0 (and of3d_last_error's text) on a
 * refusal: a null pointer, an invalid box, more than 16 boxes, no field bit set (or bits beyond
 * the four and the skip bits of the boxes), every box skipped, a workgroup share of 2^31 elements
 * or more.  of3d_field_export refuses the same, a missing pointer, a d_result that is not 16-byte
 * aligned, a mask_mode outside 0..3, and the vz bit in a 2D call (-1). */
#define OF3D_EXPORT_HEAD_WORDS 8
#define OF3D_EXPORT_ROI_WORDS 6
#define OF3D_EXPORT_SKIP_SHIFT 16
size_t of3d_field_export_result_bytes(const int64_t* rois, int n_roi, int fields, int v_f32, int rel_f64, int out_f32);
int of3d_field_export(const void* d_vx, const void* d_vy, const void* d_vz, const void* d_rel, int v_f32, int rel_f64,
                      int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                      double tscale, const int64_t* rois, int n_roi, int fields /* bit 0 vx, 1 vy, 2 vz, 3 rel */,
                      int mask_mode, int physical, int out_f32, const uint16_t* d_keep /* NULL: rel > *d_thresh */,
                      void* d_result, void* stream);

/* Projection maps: per box of the frame summary and per axis a (z, y or x) one value per line of
 * the box — the box's voxels that share the other two coordinates, taken in ascending order along
 * a — so that a summary-only series can still return the picture every figure script draws its
 * vectors on (max(myo,[],3) in plot_figure3_ROIfigures.m:298,313, plot_figure3_ChannelCompare.m:64,69
 * and plot_figure5.m:915-917; sum(relMask,3) in plot_figure4_timeTraces.m:103, plot_figure5.m:90 and
 * plot_figure5_Movie.m:91) and a 3D flow as a 2D vector map.  Fields, d_rel, dtypes, dims, d_thresh,
 * scales and rois as of3d_flow_summary's; d_keep as of3d_quiver_sample's (NULL: the mask factor is
 * rel > *d_thresh, else bit r of d_keep for box r; d_rel and d_thresh may then be NULL).  2D:
 * d_vz == NULL and nz == 1 (a d_vz with nz == 1 is an error); the axes are then y and x only.
 * axes: bit 0 z, 1 y, 2 x, one at least.  A map's plane has the box's two remaining extents in C
 * order: axis z (dy, dx), axis y (dz, dx), axis x (dz, dy).
 * maps: the maps produced, one at least; bit OF3D_PROJECT_SKIP_SHIFT + r: box r is listed but not
 * projected — it keeps its index, and so its bit of d_keep, and takes no space.  Per voxel k of a
 * line: m_k the mask factor; the physical velocity of3d_flow_summary's (v * m, an exact zero ->
 * NaN, (v * scale) / tscale); valid <=> the magnitude's square is not NaN; magnitude = its root.
 *   bit 0  n_mask         int64    the k with m_k = 1 (sum(relMask,3): a voxel inside the mask whose
 *                                  velocity is an exact zero counts here and not in n_valid)
 *   bit 1  n_valid        int64    the valid k
 *   bit 2..4 sum_vx, sum_vy, sum_vz  float64  s = 0.0; for k ascending: if valid: s = s + v_k
 *                                  (sum_vz: 3D only)
 *   bit 5  sum_magnitude  float64  the same sequential sum of the magnitudes
 *   bit 6  max_magnitude  float64  the largest magnitude of the valid k; NaN without one
 *   bit 7  max_image      float64  m = NaN; for every k: m = fmax(m, (double)image_k) — a float
 *                                  image's NaNs are ignored; the sign of a zero maximum is unspecified
 *   bit 8  sum_image      float64  s = 0.0; for every k ascending: s = s + (double)image_k (unmasked)
 * Every sum is that loop, one fp64 addition per step and no FMA contraction: a map depends on the
 * inputs alone, never on the launch shape.  Bits 7 and 8 need d_image: a volume of the same dims of
 * any of3d_dtype, read by image_dtype (uint16 / uint32 frames kept in signed storage are read as
 * the unsigned values the code names).  Without those bits d_image is not read.
 *
 * Result (device, of3d_flow_project_result_bytes(...) bytes, 8-byte words; d_result 16-byte aligned):
 *   word 0        the threshold as float64 (NaN without a d_thresh)
 *   words 1..7    n_roi, axes, maps, has_vz, the image dtype code (0 without an image map), the
 *                 total word count, 0 (int64)
 *   then per box, 6 words: for axis z, y, x the plane's element count and the word offset of the
 *   first map of (box, axis) — 0: not produced (a skipped box, an axis not asked for)
 *   then the maps, box by box, axis by axis and in bit order: each starts on a 16-byte boundary,
 *   holds the plane's elements in C order and is padded to whole 16 bytes with zeros — the maps of
 *   one (box, axis) are ((count + 1) & ~1) words apart.
 * Every byte of the result is written by the call, and nothing outside it.  Up to three launches on
 * `stream`: axes z and y in one, grid (one-wave workgroups, box, axis), one lane per line with the plane's
 * pixels flattened in C order over the lanes (consecutive lanes read consecutive x), a lane
 * marching its line four voxels per trip; axis x, grid (workgroups, box): a workgroup takes 32
 * consecutive lines and walks them 32 voxels of x per step — the tile is loaded coalesced along x,
 * the loading lane forms the voxel's physical values and parks them in LDS, and one lane per
 * (line, accumulator) adds the parked columns in ascending x; and a one-workgroup launch for the
 * header and the pads.  Every output word has one writer: no atomics, no workspace, no host copy,
 * no host synchronisation, no workgroup waits for another.
 * of3d_flow_project_result_bytes: host arithmetic only; 0 (and of3d_last_error's text) on a
 * refusal: a null pointer, an invalid box, more than 16 boxes, no axis or map bit set (or bits
 * beyond them and the skip bits of the boxes), every box skipped, the z axis or sum_vz without
 * has_vz, an image map without an image_dtype, an image_dtype that is no of3d_dtype, a box that
 * needs 2^24 workgroups or more along an axis (64 lines each for z and y, 32 for x).  of3d_flow_project refuses the same, a missing pointer, and a
 * d_result that is not 16-byte aligned (-1). */
#define OF3D_PROJECT_HEAD_WORDS 8
#define OF3D_PROJECT_ROI_WORDS 6
#define OF3D_PROJECT_SKIP_SHIFT 16
size_t of3d_flow_project_result_bytes(const int64_t* rois, int n_roi, int axes, int maps, int has_vz, int image_dtype);
int of3d_flow_project(const void* d_vx, const void* d_vy, const void* d_vz, const void* d_rel, int v_f32, int rel_f64,
                      int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                      double tscale, const int64_t* rois, int n_roi, int axes /* bit 0 z, 1 y, 2 x */, int maps,
                      const void* d_image /* NULL: no image maps */, int image_dtype,
                      const uint16_t* d_keep /* NULL: rel > *d_thresh */, void* d_result, void* stream);

/* Contractility: the flow with respect to the centroid of the mask, on the device — the
 * reference's figure 2 / movie S2 (plot_figure2_movie.ipynb cell 1: com = center_of_mass(relMask),
 * normalc = -(pos - com) / |pos - com| in physical units, vnorm = v / |v|,
 * degrees(arccos(vecdot(vnorm, normalc)))): 0 degrees is a velocity straight towards the centroid
 * (contracting), 180 straight away from it.  Fields, d_rel, dtypes, dims, d_thresh, scales, rois
 * and validity as of3d_flow_summary's; d_keep as of3d_flow_whist's (NULL: rel > *d_thresh; else bit
 * r of d_keep for box r — of3d_mask_largest's output for the figure —, and d_rel / d_thresh may
 * then be NULL).  2D: d_vz == NULL and nz == 1 (a d_vz with nz == 1 is an error); every z term is
 * dropped.  For every box r independently:
 *   1. the mask M_r of of3d_mask_axes step 1 (the mask, not the valid voxels) and its unsigned
 *      64-bit sums n, Sx, Sy, Sz of the box-local integer coordinates, by of3d_mask_axes' own
 *      moment pass; the centroid c = S / n in box-local index coordinates, one float64 division of
 *      two integers exact in float64 — scipy.ndimage.center_of_mass of the integer mask, bit for
 *      bit.  n == 0: NaN, and no voxel then has an angle.
 *   2. the centre used: c, or center_given (host, 3 finite doubles x y z, box-local, the same for
 *      every box; kernel arguments).  Step 1 is reported either way.  The centre is written into
 *      the result on the device and read from there by the reduction, later on the same stream.
 *   3. per valid voxel at box-local integer coordinates (kx, ky, kz), with (vx, vy, vz) its masked
 *      physical velocity, plain multiplies and adds in this order (no FMA):
 *        dx = kx*xyscale - c.x*xyscale   dy = ky*xyscale - c.y*xyscale   dz = kz*zscale - c.z*zscale
 *        nd = sqrt((dx*dx + dy*dy) + dz*dz)      speed = sqrt((vx*vx + vy*vy) + vz*vz)
 *        dot = ((vx/speed)*(-dx/nd) + (vy/speed)*(-dy/nd)) + (vz/speed)*(-dz/nd)
 *        angle = acos(min(max(dot, -1), 1)) * (180/pi)          inward = speed * dot
 *      inward is the physical velocity component towards the centre.  The voxel with nd == 0 (the
 *      centre's own) has a NaN direction: it counts in n_valid, not in n_angle.
 * Not reproduced of the notebook: numpy's arccos returns NaN where rounding leaves |dot| a last
 * bit above 1; here dot is clamped first, so such a voxel has exactly 0 or 180 degrees (and
 * counts in n_angle and the sums; dot itself is summed unclamped).
 *
 * Result (device, of3d_flow_contract_result_bytes(n_roi, nbins2) bytes, 8-byte words, zeroed on
 * the stream first), per box OF3D_CONTRACT_ROI_WORDS + sum(nbins2) words:
 *    0..3    uint64 n, Sx, Sy, Sz
 *    4..6    float64 centroid x y z, box-local (add the box origin for volume coordinates)
 *    7..9    float64 the centre used x y z, box-local
 *   10..12   int64 n_valid, n_angle, n_inward (voxels with dot > 0)
 *   13..16   float64 sums over the voxels with an angle: angle, dot, inward, speed
 *   17..     uint64 histogram counts of angle (degrees), then inward (nbins2[q] words each;
 *            np.histogram semantics, at most 256 bins, edges2: host double*[2]; all 0 is legal)
 * Deterministic under of3d_flow_summary's contract: its workgroup partition and walk, the sums in
 * registers, a fixed shuffle tree over the lanes, the waves in wave order into the workgroup's own
 * workspace slot, a second kernel adding a box's slots in index order; counts and histograms by
 * integer atomics; no floating-point atomic.  Equal inputs give equal bits on every run, and a
 * box's words do not depend on the other boxes.
 * `workspace`: device memory of of3d_flow_contract_workspace_bytes(rois, n_roi, nbins2) bytes (the
 * moment pass's block and workspace, the edges, one slot of 4 float64 per workgroup of every
 * box); host arithmetic only, 0 (and of3d_last_error's text) for an invalid box, more than 16
 * boxes, more than 256 bins, a workgroup share of 2^31 voxels or more, or a box whose sums could
 * pass 2^63 (of3d_mask_axes_workspace_bytes' rule).  Enqueued on `stream`; no host copy, no host
 * synchronisation, no workgroup waits for another. */
#define OF3D_CONTRACT_QUANTITIES 2 /* histograms: 0 angle, 1 inward */
#define OF3D_CONTRACT_ROI_WORDS 17
size_t of3d_flow_contract_result_bytes(int n_roi, const int* nbins2);
size_t of3d_flow_contract_workspace_bytes(const int64_t* rois, int n_roi, const int* nbins2);
int of3d_flow_contract(const void* d_vx, const void* d_vy, const void* d_vz, const void* d_rel, int v_f32, int rel_f64,
                       int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                       double tscale, const int64_t* rois, int n_roi, const uint16_t* d_keep,
                       const double* center_given, const int* nbins2, const double* const* edges2, void* d_result,
                       void* workspace, void* stream);

/* Spread of the flow about a centre: per box the second moments of the deviations of vx, vy, vz
 * and the magnitude from a centre, the sums of sin / cos of phi, and the extremes — what the
 * reference's validation figure reduces a frame to (plot_FigureS1_translation.ipynb, cell
 * "Calculations over time": np.nanstd of vx, vy, vz and the speed, the circular standard
 * deviation of theta and of phi, set against the translation applied to the images), and the
 * extremes the other figures pick their colour limits from.  Fields, d_rel, dtypes, dims,
 * d_thresh, scales, rois and validity (magnitude not NaN) as of3d_flow_summary's; d_keep as
 * of3d_flow_whist's (NULL: rel > *d_thresh; else bit r of d_keep for box r, and d_rel / d_thresh
 * may then be NULL).  2D: d_vz == NULL and nz == 1; every vz term is 0 and the phi sums are 0.
 * The centre (vx, vy, vz, magnitude; physical units):
 *   center == NULL  box r is measured about its own mean c_q = sum_q / n_valid, one float64
 *                   division on the device from d_summary, the device result of
 *                   of3d_flow_summary[_masked] for the same inputs (enqueued earlier on `stream`;
 *                   summary_nbins: that call's nbins, host int[6], which place a box's words).
 *                   Nothing returns to the host.  n_valid == 0 gives a NaN centre.
 *   center given    host, 4 doubles, the same for every box (kernel arguments) — deviations from
 *                   a known velocity; d_summary and summary_nbins may then be NULL.  2D: center[2]
 *                   is taken as 0.
 * A pass of its own because the deviations must be centred: the one-pass form E[x^2] - E[x]^2
 * cancels where the spread is small against the mean (a near-uniform translation), and the mean
 * exists only after the summary's final kernel.  Per valid voxel, with d = value - centre:
 * dvx^2, dvy^2, dvz^2, dmag^2, dvx*dvy, dvx*dvz, dvy*dvz; sin(phi) = vz / mag and cos(phi) = h / mag,
 * h = sqrt(vx^2 + vy^2) (as the summary forms sin(theta) = vy / h); the running minimum and
 * maximum of vx, vy, vz and the magnitude.
 *
 * Result (device, of3d_flow_spread_result_bytes(n_roi) bytes, 8-byte words, zeroed on the stream
 * first), per box OF3D_SPREAD_ROI_WORDS words:
 *    0       n_valid (int64; of3d_flow_summary's for the same mask)
 *    1..4    float64 the centre used: vx vy vz magnitude
 *    5..11   float64 sums of dvx^2 dvy^2 dvz^2 dmag^2 dvx*dvy dvx*dvz dvy*dvz
 *   12..13   float64 sums of sin(phi), cos(phi)
 *   14..17   float64 minima of vx vy vz magnitude (NaN when n_valid == 0)
 *   18..21   float64 maxima of vx vy vz magnitude (NaN when n_valid == 0)
 * Deterministic under of3d_flow_summary's contract: its workgroup partition and walk, the sums in
 * registers, a fixed shuffle tree over the lanes, the waves in wave order into the workgroup's own
 * workspace slot, a second kernel adding a box's slots in index order; the extremes go through
 * the same slots (a minimum does not depend on the order); n_valid by integer atomics; no
 * floating-point atomic.  Equal inputs give equal bits on every run, and a box's words do not
 * depend on the other boxes.
 * `workspace`: device memory of of3d_flow_spread_workspace_bytes(rois, n_roi) bytes (one slot of
 * 17 float64 per workgroup of every box); host arithmetic only, 0 (and of3d_last_error's text) for
 * an invalid box, more than 16 boxes or a workgroup share of 2^31 voxels or more.  Enqueued on
 * `stream`; no host copy, no host synchronisation, no workgroup waits for another. */
#define OF3D_SPREAD_ROI_WORDS 22
size_t of3d_flow_spread_result_bytes(int n_roi);
size_t of3d_flow_spread_workspace_bytes(const int64_t* rois, int n_roi);
int of3d_flow_spread(const void* d_vx, const void* d_vy, const void* d_vz, const void* d_rel, int v_f32, int rel_f64,
                     int64_t nz, int64_t ny, int64_t nx, const void* d_thresh, double xyscale, double zscale,
                     double tscale, const int64_t* rois, int n_roi, const uint16_t* d_keep, const void* d_summary,
                     const int* summary_nbins, const double* center, void* d_result, void* workspace, void* stream);

/* Percentiles of one box of rel, selected on the device: how the reference's figure scripts form
 * the reliability threshold,
 *   relCrop = rel(y0:y1, x0:x1, z0:z1);  relThresh = prctile(relCrop(:), relPer);
 * (plot_figure5.m:80-84, plot_figure5_Movie.m:81-85, plot_figure3_ROIfigures.m:70-84,
 * plot_figure3_ChannelCompare.m:114-128), without the crop's copy: the volume is read in place.
 * d_rel: (nz, ny, nx) float32 (float64 with rel_f64), 2D = nz 1.  box: host int64[6] = z0 z1 y0 y1
 * x0 x1, half-open, inside the volume and not empty; NULL: the whole volume.  n_q: 1 to
 * OF3D_SELECT_MAX percentiles, each given as of3d_quantile gives its one: host arrays lo[n_q],
 * hi[n_q] (0-based ranks among the box's n_box voxels, 0 <= lo <= hi <= n_box - 1) and
 * gamma[n_q] in [0, 1]; the caller's percentile definition decides them (numpy 'linear', or
 * 'hazen' = MATLAB's prctile).  d_out: n_q device elements of rel's dtype; element k is numpy's
 * _lerp of the two order statistics in rel's dtype, a + (b - a) * g for g < 0.5 and
 * b - (b - a) * (1 - g) otherwise — lo == hi goes through the same expression, so an infinite
 * value gives NaN as numpy does.  -0.0 and +0.0 are one value (+0.0 is returned).  A NaN inside
 * the box makes every output NaN; a NaN outside it is never read.  Ranks 0 and n_box - 1 are the
 * box's exact minimum and maximum.  d_out + k is a valid d_thresh of every pass here.
 * Radix select over 11-bit digits (float32 3 passes, float64 6): per pass one histogram per
 * distinct key prefix among the up to 16 ranks (the prefixes kept sorted: a voxel finds its
 * histogram by a range reject and a binary search), LDS integer atomics flushed by 64-bit integer
 * atomics, then one workgroup narrows every rank.  Rows of the box are walked with 16-byte loads
 * over their aligned middle and element loads at their ends; full-width rows are joined.
 * Deterministic: integer counts only, equal inputs give equal bits.  `workspace`: device memory
 * of of3d_rel_select_workspace_bytes(rel_f64) bytes.  Enqueued on `stream`; no host copy, no host
 * synchronisation, no launch shape that depends on device data. */
#define OF3D_SELECT_MAX 8
size_t of3d_rel_select_workspace_bytes(int rel_f64);
int of3d_rel_select(const void* d_rel, int rel_f64, int64_t nz, int64_t ny, int64_t nx, const int64_t* box, int n_q,
                    const int64_t* lo, const int64_t* hi, const double* gamma, void* d_out, void* workspace,
                    void* stream);

/* Reliability profile: what plot_figureS3_reliability.ipynb cells 4-8 look at to choose the
 * percentile — the thresholds at several percentiles, how many voxels each mask keeps, and the
 * distribution of rel (plt.hist(rel.flatten(), 50)) — per box, over all voxels of the box (no
 * mask).  d_rel, dims and rois (n_roi <= 16) as of3d_flow_summary's.  d_thresh: n_q (0 to
 * OF3D_SELECT_MAX) device elements of rel's dtype, e.g. of3d_rel_select's output; the comparison
 * rel > t_k is made in rel's dtype, as in every other pass.  The histogram has nbins (1 to 256)
 * bins of (double)rel with np.histogram(values, bins=edges) semantics (last bin closed, values
 * outside and NaN dropped); its edges come in exactly one of two ways:
 *   edges    host, nbins + 1 strictly ascending values without NaN (kernel arguments);
 *   d_range  two device elements lo, hi of rel's dtype (of3d_rel_select's outputs for ranks 0 and
 *            n_box - 1): a kernel forms np.linspace(lo, hi, nbins + 1) in float64 — step =
 *            (hi - lo) / nbins, e_i = i * step + lo (a multiply, then an add), e_nbins = hi; lo ==
 *            hi is widened to lo - 0.5, hi + 0.5 first (np.histogram's outer edges).  A NaN or
 *            infinite lo / hi gives NaN edges and all-zero counts, where numpy raises.
 * Result (device, of3d_rel_profile_result_bytes(n_roi, n_q, nbins) bytes, 8-byte words, zeroed on
 * the stream first):
 *   word 0  n_roi    word 1  n_q    word 2  nbins   (uint64; OF3D_PROFILE_HEAD words)
 *   then n_q words: the thresholds as float64
 *   then nbins + 1 words: the edges used (float64)
 *   then per box, 2 + n_q + nbins words:
 *     0  n_voxels    1  n_nan    2..  n_above[k] = #{rel > t_k}    then hist[nbins]   (uint64)
 * Deterministic: of3d_flow_summary's workgroup partition and walk, per-thread integer counters
 * reduced per wave, an LDS histogram, 64-bit integer atomics; no floating-point accumulation
 * anywhere, so equal inputs give equal bits on every run and a box's words do not depend on the
 * other boxes.  Enqueued on `stream`; no host copy, no host synchronisation. */
#define OF3D_PROFILE_HEAD 3
size_t of3d_rel_profile_result_bytes(int n_roi, int n_q, int nbins);
int of3d_rel_profile(const void* d_rel, int rel_f64, int64_t nz, int64_t ny, int64_t nx, const int64_t* rois,
                     int n_roi, const void* d_thresh, int n_q, int nbins, const double* edges, const void* d_range,
                     void* d_result, void* stream);

/* Reliability (smallest eigenvalue) of n given symmetric 3x3 structure tensors
 * resident on the device: `tensor` is field-major [6][n] float64 in the order
 * x2 y2 z2 xy xz yz (calc_flow.py:352-354's matrix (x2 xy xz / xy y2 yz /
 * xz yz z2)); `rel` receives float32 (the reference's complex64 cgeev
 * precision, calc_flow.py:355-357) or, with rel_f64, float64 (MATLAB's double
 * pageeig, M/calc_flow3D.m:235-236) — exactly the values the flow kernels
 * store for those tensors.  Enqueued on `stream`. */
int of3d_rel3d(const double* tensor, int64_t n, void* rel, int rel_f64, void* stream);

/* Fill the plan's device workspace (both field buffers) with `byte` on `stream`, and forget every
 * temporal derivative an earlier call formed for a later one (execute_next's, execute_ahead's
 * slots): the next execute call recomputes.  plan == NULL: the same for every plan the host
 * entry points cache, their input and output staging included (synchronous).  Results of later
 * calls must not change: between calls the workspace carries nothing but those tagged
 * derivatives.  `byte` in [0, 255]; 0xFF makes every fp64 and fp32 element a NaN.  Returns 0 for
 * a plan, the number of cached plans filled for NULL, negative on error.  For tests (no
 * reference counterpart); never called on a product path. */
int of3d_plan_poison(of3d_plan* plan, int byte, void* stream);

/* Blocking copy of n buffers on the GPU's DMA (SDMA) engines through the HSA
 * runtime: no compute units and no HIP stream involved, so a download does
 * not contend with kernels for the memory pipeline.  Host buffers must be
 * pinned.  The caller orders it after the producing work (e.g. a download
 * thread after hipEventSynchronize).  Releases no locks of its own; safe to
 * call from several threads. */
int of3d_dma_copy(void* const* dst, const void* const* src, const size_t* bytes, int n);

#ifdef __cplusplus
}
#endif
#endif /* OF3D_H */

/*
 * slamhip.h — C-ABI of the MI355X-native ICP + SE(2) pose-graph hot path.
 *
 * Drop-in boundary for cohnt/ICP-SLAM-with-Loop-Closure (reference at
 * /root/reference).  The reference is pure Python/NumPy, so its "FFI" for this
 * path is the Python call surface of src/icp.py and
 * src/pose_graph_optimization.py; the build's drop-in modules
 * (the .py modules in icp-slam-with-loop-closure_amd/src) bind these entry points with
 * ctypes.  Each entry point names the reference
 * function(s) it replaces.
 *
 * Conventions (all entry points):
 *   - every array argument is a DEVICE pointer (hipMalloc / torch-ROCm
 *     storage) owned by the caller; scalars are host values;
 *   - points are packed (x, y) float64 pairs ("double2"); the homogeneous
 *     coordinate of the reference's (n, 3) arrays is implicit and must be 1
 *     (np.c_[points, ones] as scripts/main.py:242-243 builds them);
 *   - 3x3 SE(2) matrices are 9 float64, row-major, last row [0, 0, 1];
 *   - launches are asynchronous and ordered on `stream` (a hipStream_t; NULL
 *     = the legacy default stream) and copy nothing to the host; nothing is
 *     allocated persistently.  One exception to "allocates nothing": a
 *     slam_icp_batch_f64 call of >= 1024 pairs takes a transient
 *     stream-ordered workspace (hipMallocAsync / hipFreeAsync, 12 B per pair),
 *     which stream capture records as graph memory nodes;
 *   - return 0 on success, a negative SLAM_E* code on failure; the message is
 *     available from slam_last_error() (thread-local);
 *   - the tuning and diagnostics switches (slam_icp_set_*, slam_gn_set_*)
 *     are per host thread (thread-local, like slam_last_error): a thread's
 *     settings never change another thread's launches;
 *   - one host thread per device at a time: the batch scheduler's side
 *     streams and fork / join events are one set per device.
 */
#ifndef SLAMHIP_H
#define SLAMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_OK 0
#define SLAM_EINVAL (-1)   /* bad shape / argument */
#define SLAM_EHIP (-2)     /* HIP runtime error (launch, device) */
#define SLAM_ETOOBIG (-3)  /* a scan larger than the compiled query capacity */

/* Library identity: ABI version (major*100 + minor). */
int slam_abi_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* slam_last_error(void);
/* Largest query scan (pc1) one workgroup can hold (points). */
int slam_icp_max_query_points(void);

/*
 * Batched ICP, one scan pair per workgroup, all iterations on chip.
 * Replaces src/icp.py:72-97 `icp(pc1, pc2, init_transform, epsilon,
 * max_iters, stopping_thresh, rotation_only)` for B independent pairs, i.e.
 * the joblib fan-out of scripts/main.py:240-247,
 * src/pose_graph_optimization.py:59-68 and src/loop_closure_detection.py:134-142.
 *
 *   pts       all scans, packed double2, scan s = pts[scan_off[s] .. scan_off[s+1])
 *   scan_off  int64[n_scans + 1]
 *   src_scan  int32[B]  pc1 (moving/query cloud) of pair b
 *   dst_scan  int32[B]  pc2 (reference cloud) of pair b
 *   init      float64[B][9] initial transforms
 *   max_n1/max_n2  host upper bounds of the pc1 / pc2 sizes in this batch
 *                  (select the kernel instance and LDS size).  The kernel
 *                  checks every pair against them: a pair with an empty scan
 *                  or n1 > max_n1's instance capacity or n2 > max_n2's LDS
 *                  capacity is not computed (out_iters = INT32_MIN, out_err =
 *                  NaN) and raises the flag slam_icp_status() reports
 *   hist_stride    0, or >= max_iters + 3: out_hist[b] holds the full
 *                  transform list [init, T1, ..., T_k] the reference returns
 *   out_hist  float64[B][hist_stride][9] (NULL if hist_stride == 0)
 *   out_tf    float64[B][9]  final transform (transforms[-1])
 *   out_err   float64[B]     returned error (of the penultimate transform)
 *   out_iters int32[B]       number of ICP iterations k (len(transforms) - 1)
 * Stopping rules are the reference's: err < epsilon; iteration > max_iters;
 * |last_err - err| < stopping_thresh from the second iteration on.
 * Batches of >= 1024 pairs run in two phases (slam_icp_set_schedule) with a
 * transient stream-ordered workspace of 12 B/pair (hipMallocAsync/FreeAsync).
 */
int slam_icp_batch_f64(const double* pts, const int64_t* scan_off,
                       const int32_t* src_scan, const int32_t* dst_scan,
                       const double* init, int32_t B,
                       double epsilon, int32_t max_iters, double stopping_thresh,
                       int32_t rotation_only, int32_t max_n1, int32_t max_n2,
                       int32_t hist_stride, double* out_hist, double* out_tf,
                       double* out_err, int32_t* out_iters, void* stream);

/*
 * Synchronises `stream` and reports the device-side bounds check of every
 * slam_icp_batch_f64 / slam_icp_step_f64 launch since the previous call:
 * SLAM_OK, or SLAM_EINVAL when some pair was outside its launch's max_n1 /
 * max_n2 (see above); the flag is then cleared.
 */
int slam_icp_status(void* stream);

/*
 * One ICP iteration per pair.  Replaces src/icp.py:55-69 `icp_iteration(pc1,
 * pc2, previous_transform, rotation_only)`; with T_in = identity it is
 * src/icp.py:10-19 `get_correspondences(pc1, pc2)` (an identity transform
 * reproduces the query coordinates exactly).
 *   T_in      float64[B][9]
 *   T_out     float64[B][9]   transform @ previous_transform
 *   out_corr  int64[...]      correspondences of pair b written at
 *                             out_corr[corr_off[b] + i], i < n1(b)
 *   corr_off  int64[B]
 *   out_err   float64[B]      get_error of the pre-update cloud
 */
int slam_icp_step_f64(const double* pts, const int64_t* scan_off,
                      const int32_t* src_scan, const int32_t* dst_scan,
                      const double* T_in, int32_t B, int32_t rotation_only,
                      int32_t max_n1, int32_t max_n2, double* T_out,
                      int64_t* out_corr, const int64_t* corr_off,
                      double* out_err, void* stream);

/*
 * Rigid 2-D fit of matched rows a[i] -> b[i] (n rows each, double2).
 * Replaces src/icp.py:22-46 `get_transform(pc1, pc2)` (out_T) and
 * src/icp.py:49-52 `get_error(pc1, pc2)` (out_err, the SUM of squares).
 */
int slam_kabsch2d_f64(const double* a, const double* b, int64_t n,
                      double* out_T, double* out_err, void* stream);

/*
 * One stochastic-gradient relaxation step, in place on poses (N x 3).
 * Replaces src/pose_graph_optimization.py:7-49
 * `pose_graph_optimization_step_sgd(pose_graph, learning_rate,
 * loop_closure_uncertainty)`.  Edges (ea[e] -> eb[e], tf[e] 3x3) must be in
 * the pose graph's networkx iteration order; |a-b| == 1 edges are skipped as
 * in the reference.  `work`: float64[slam_pgo_sgd_work_size(N, E)] scratch.
 */
int slam_pgo_sgd_step_f64(double* poses, int32_t N, const int32_t* ea,
                          const int32_t* eb, const double* tf, int32_t E,
                          double learning_rate, double loop_closure_uncertainty,
                          double* work, void* stream);

/* float64 elements of the `work` scratch slam_pgo_sgd_step_f64 needs. */
int64_t slam_pgo_sgd_work_size(int32_t N, int32_t E);

/*
 * What slam_pgo_sgd_step_f64 launches for the relaxation of N >= 1 poses (host
 * only; the step chooses its launch through the same function): *in_lds 1 =
 * one wave with the poses in LDS, 0 = a workgroup with the poses in global
 * memory; *rounds = whole-block update rounds of the one-wave kernel (BR, 1 or
 * 2; 1 on the workgroup path); *shift = log2 of the lazy-offset block size;
 * *threads = the launch's thread count.  Any output pointer may be NULL.
 * Reports the forced plan while slam_pgo_sgd_force is active, SLAM_EINVAL if
 * that setting cannot hold N poses.
 */
int slam_pgo_sgd_plan(int32_t N, int32_t* in_lds, int32_t* rounds, int32_t* shift, int32_t* threads);

/*
 * Diagnostics / tests: force the relaxation's launch.  path: -1 automatic, 0
 * one wave BR = 1, 1 one wave BR = 2, 2 workgroup with global poses.  shift: -1
 * automatic, or 6..12, accepted with path == 2 only (the one-wave kernel has
 * 128 explicit-node slots: shift 6).  A step whose forced setting cannot hold
 * its graph (N above the LDS pose capacity, more blocks than 64 * BR or than
 * the lazy-offset table) returns SLAM_EINVAL before launching anything.  Per
 * host thread; results agree to rounding between paths.
 */
int slam_pgo_sgd_force(int32_t path, int32_t shift);

/*
 * Heading recompute from positions, in place.  Replaces the first loop of
 * src/pose_graph_optimization.py:51-57 `recompute_pose_graph_orientation`.
 */
int slam_pgo_orient_f64(double* poses, int32_t N, void* stream);

/*
 * Second half of recompute_pose_graph_orientation with icp_recompute
 * (src/pose_graph_optimization.py:68-74): theta_i = theta_{i-1} +
 * atan2(tf_i[1,0], tf_i[0,0]) for i = 1..N-1, theta_{i-1} taken BEFORE its
 * own update (the reference's reverse-order loop).  tf: float64[N-1][9]
 * rotation-only ICP results of pairs (i, i-1); work: float64[N].
 */
int slam_pgo_orient_from_tf_f64(double* poses, int32_t N, const double* tf,
                                double* work, void* stream);

/*
 * One Gauss-Newton iteration of the SE(2) pose graph (north-star solve; the
 * reference has only the SGD relaxation).  Problem: the graph as
 * src/pose_graph.py:61-73 exports it to g2o — edge e: ea[e] -> eb[e] with
 * relative measurement tf[e] and isotropic information w[e]; node columns
 * node_col[n] (-1 = fixed) in a bandwidth-reducing order; H lower band of
 * half-width W scalars; slot_* list the edge contributions of every H block
 * (see slamhip/gn.py GnPlan).  Poses are updated in place; chi2 before the
 * step -> *out_chi2 (device); *status != 0 if H was not positive definite.
 */
int64_t slam_gn_work_size(int32_t N, int32_t E, int32_t W);
int slam_gn_max_lds_band(void);
int slam_gn_iteration_f64(double* poses, int32_t N, const int32_t* ea,
                          const int32_t* eb, const double* tf, const double* w,
                          int32_t E, const int32_t* node_col,
                          const int32_t* slot_rc, const int32_t* slot_ptr,
                          const int32_t* slot_items, int32_t n_slots,
                          int32_t nv, int32_t W, double* work,
                          double* out_chi2, int32_t* status, void* stream);

/*
 * The same iteration for a band + border plan (slamhip/gn.py GnPlan with a
 * border, e.g. C4's lap graph cut at one place): scalars [0, nv_band) form
 * the band of half-width W, the last nv - nv_band <= 31 scalars a border
 * coupled to band rows nbr_rows[0..n_nbr) only.  Solved as H = [A B; B^T C]:
 * Z = A^-1 [r_a | B] by block cyclic reduction with several right-hand
 * sides, S = C - B^T Z_B, x_b = S^-1 (r_b - B^T Z_r), x_a = Z_r - Z_B x_b.
 * work: slam_gn_work_size_bordered(N, E, W, nv - nv_band) doubles.
 */
int64_t slam_gn_work_size_bordered(int32_t N, int32_t E, int32_t W,
                                   int32_t n_border);
int slam_gn_iteration_bordered_f64(double* poses, int32_t N, const int32_t* ea,
                                   const int32_t* eb, const double* tf,
                                   const double* w, int32_t E,
                                   const int32_t* node_col,
                                   const int32_t* slot_rc,
                                   const int32_t* slot_ptr,
                                   const int32_t* slot_items, int32_t n_slots,
                                   int32_t nv, int32_t W, int32_t nv_band,
                                   const int32_t* nbr_rows, int32_t n_nbr,
                                   double* work, double* out_chi2,
                                   int32_t* status, void* stream);
/* The same bordered iteration with the border's Schur complement accumulated
 * DURING the band's elimination: every eliminated
 * block i with pslot[i] = k >= 0 (the blocks whose reduced rows couple to the
 * border; slamhip.gn.GnPlan lists them symbolically) adds Y_i^T D_i^-1 Y_i to
 * slot k of pwork (n_pslot x mc x mc doubles, mc = 16 ceil((nbd + 1) / 16)),
 * the top block forms S and x_b = S^-1 s, and the back-substitution runs on
 * one column.  Same result as slam_gn_iteration_bordered_f64 to rounding;
 * needs the explicit-inverse cyclic reduction (SLAM_EINVAL otherwise).
 * The back-substitution runs as ONE XCD-local launch by default
 * (slam_gn_set_fused_back): a fused wait that timed out sets *status |= 2,
 * the step is then invalid and is re-run with slam_gn_set_fused_back(0)
 * (slamhip.gn does this).
 * work: slam_gn_work_size_bordered(N, E, W, nv - nv_band) doubles. */
int slam_gn_iteration_schur_f64(double* poses, int32_t N, const int32_t* ea,
                                const int32_t* eb, const double* tf,
                                const double* w, int32_t E,
                                const int32_t* node_col,
                                const int32_t* slot_rc,
                                const int32_t* slot_ptr,
                                const int32_t* slot_items, int32_t n_slots,
                                int32_t nv, int32_t W, int32_t nv_band,
                                const int32_t* pslot, int32_t n_pslot,
                                double* pwork, double* work,
                                double* out_chi2, int32_t* status,
                                void* stream);
/* The Schur path's back-substitution: one XCD-local launch (1, default) or
 * one launch per level (0). */
int slam_gn_set_fused_back(int on);
int slam_gn_get_fused_back(void);
/* 1 when slam_gn_iteration_schur_f64 can run in this process (the
 * explicit-inverse cyclic reduction is the solver: not with
 * slam_gn_set_solver(1) or the SLAMHIP_BCR_CHOL / SLAMHIP_BCR_LEGACY A/B
 * switches), 0 otherwise: a bordered plan then takes
 * slam_gn_iteration_bordered_f64. */
int slam_gn_schur_supported(void);
/* Diagnostics (host only; new since ABI 102): which of the cyclic reduction's
 * A/B switches this process latched from its environment, as a bitmask.  Each
 * switch is read once, at its first use or at this call, whichever is first:
 *   SLAM_GN_VARIANT_CHOL        SLAMHIP_BCR_CHOL=1 (Cholesky paths)
 *   SLAM_GN_VARIANT_LEGACY      SLAMHIP_BCR_LEGACY=1 (register elimination)
 *   SLAM_GN_VARIANT_ODD_MFMA    SLAMHIP_BCR_ODD_MFMA=1 (blocked MFMA odd kernel)
 *   SLAM_GN_VARIANT_SPLIT       SLAMHIP_GN_SPLIT_MIN=n with n > 0 (levels of at
 *                               least n odd blocks invert them once, in place)
 *   SLAM_GN_VARIANT_FUSED_BACK  the fused back-substitution's default is on
 *                               (off with SLAMHIP_GN_FUSED_BACK=0;
 *                               slam_gn_set_fused_back changes the current
 *                               setting, not this bit)
 * A default process returns SLAM_GN_VARIANT_FUSED_BACK. */
#define SLAM_GN_VARIANT_CHOL 1
#define SLAM_GN_VARIANT_LEGACY 2
#define SLAM_GN_VARIANT_ODD_MFMA 4
#define SLAM_GN_VARIANT_SPLIT 8
#define SLAM_GN_VARIANT_FUSED_BACK 16
int slam_gn_bcr_variant(void);
/* Diagnostics: the fused back-substitution's longest wait in s_memrealtime
 * ticks (0: the default 0.2 s); a tiny wait forces the timeout path. */
int slam_gn_set_fused_wait(uint32_t ticks);

/*
 * Robust loss kernels for the Gauss-Newton iterations above, by per-edge
 * reweighting (new since ABI 110).  One launch, one
 * thread per edge, at the current poses: s_e = info[e] |e_e|^2 with the same
 * residual e_e as the iteration's linearisation, the ratio r_e = rho'(s_e) of
 * the loss (1 where robust_mask[e] == 0), and
 *   w_out[e] = info[e] r_e          the array the next iteration reads as w
 *   s_out[e] = s_e, ratio_out[e] = r_e
 *   cost_partials[g], smax_partials[g]   per workgroup g of
 *       SLAM_GN_ROBUST_BLOCK edges ((E + 255) / 256 of each): the sum of
 *       rho(s_e) over the masked edges plus s_e over the others, in a fixed
 *       order, and the largest masked s_e (0 without one).
 * loss: SLAM_LOSS_*; c > 0 is the loss scale in units of sqrt(info) x
 * residual, c2 = c^2; mu >= 1 scales c2 for SLAM_LOSS_GNC_GM (graduated
 * non-convexity, the caller lowers mu towards 1) and is ignored otherwise:
 *   huber    r = 1 (s <= c2), else c / sqrt(s)
 *   cauchy   r = 1 / (1 + s / c2)
 *   gm       r = (c2 / (c2 + s))^2             (Geman-McClure)
 *   dcs      r = min(1, 2 c2 / (c2 + s))^2     (dynamic covariance scaling)
 * Arguments are checked before the launch (SLAM_EINVAL); E == 0 does nothing.
 */
#define SLAM_LOSS_HUBER 0
#define SLAM_LOSS_CAUCHY 1
#define SLAM_LOSS_GM 2
#define SLAM_LOSS_DCS 3
#define SLAM_LOSS_GNC_GM 4
#define SLAM_GN_ROBUST_BLOCK 256
int slam_gn_robust_weights_f64(const double* poses, const int32_t* ea,
                               const int32_t* eb, const double* tf,
                               const double* info, const uint8_t* robust_mask,
                               int32_t E, int32_t loss, double c, double mu,
                               double* w_out, double* s_out, double* ratio_out,
                               double* cost_partials, double* smax_partials,
                               void* stream);

/* ---- occupancy grid (src/produce_occupancy_grid.py) ------------------------
 * pts: packed (x, y) scan points, scan_off (S+1), pose4 (S x 4: cos theta,
 * sin theta, x, y of each scan's pose; cos/sin as np.cos/np.sin give them).
 * slam_grid_global_points_f64 replaces construct_global_points (:75-87):
 * gpts (P x 2) and bounds = (min x, max x, min y, max y) of all of them.
 * slam_grid_update_i8 replaces update_occupancy_grid / the beam loop of
 * produce_occupancy_grid (:54-73, bresenham_update :89-121): the int8 grid
 * (H x W, row = y) is updated in place with the reference's per-beam rule.
 * work: slam_grid_work_size(S, H, W) BYTES. */
int64_t slam_grid_work_size(int32_t S, int32_t H, int32_t W);
int slam_grid_global_points_f64(const double* pts, const int64_t* scan_off, int32_t S, const double* pose4,
                                double* gpts, double* bounds, void* work, void* stream);
int slam_grid_update_i8(const double* gpts, const int64_t* scan_off, int32_t S, const double* pose4, int64_t P,
                        double min_x, double min_y, double cell_width, int32_t H, int32_t W, int32_t k_hit,
                        int32_t k_miss, int8_t* grid, void* work, void* stream);

/* ---- correlative scan matcher (csrc/csm_kernels.hip) -----------------------
 * A brute-force, single-resolution correlative scan match (Olson 2009) of B
 * scan pairs: an initial guess for loop-closure ICP that does not need the two
 * scans to share a heading.  The reference has no counterpart (it starts every
 * loop-closure ICP from identity); new since ABI 101.
 *   pts, scan_off, src_scan (query q), dst_scan (reference r): as
 *             slam_icp_batch_f64; the match follows icp(pc1 = q, pc2 = r),
 *             a transform T with T q ~ r
 *   centre    float64[B][3]  search centre (theta0, tx0, ty0) of pair b
 *   rot       float64[B][n_theta][2]  (cos, sin) of theta_k = theta0 +
 *             (k - n_theta / 2) d_theta, evaluated by the caller (np.cos /
 *             np.sin of the Python float, like pose4 above)
 *   res, G    cell width and cells per side (even) of the look-up table; its
 *             origin is -(G / 2) res on both axes
 *   nx, ny    shift window in cells (any parity)
 * Table L (G x G, row = y): 2 on every cell floor((p - origin) / res) that
 * holds a reference point, 1 on the 8 neighbours of such a cell that hold
 * none, 0 elsewhere (each of the 9 cells clipped on its own).  Query cells per
 * angle: X = (c x - s y) + tx0, Y = (s x + c y) + ty0, ix = floor((X - origin)
 * / res), iy likewise (true fp64 division, no contraction).  Score
 * S[k][j][i] = sum over query points of L[iy + j - ny / 2][ix + i - nx / 2],
 * a cell outside the grid (or beyond int32) adding 0.  Only integers are
 * summed: the result does not depend on summation order or launch shape.
 *   out_best    int32[B][4]  maximum score, then k, j, i of the maximum with
 *               the smallest flat index (k ny + j) nx + i
 *   out_scores  int32[B][n_theta][ny][nx] the whole volume, or NULL
 *   work        slam_csm_work_size(B, G, n_theta, ny, nx) BYTES
 * The caller assembles T from (c_k, s_k) and tx0 + (i - nx / 2) res, ty0 +
 * (j - ny / 2) res.  SLAM_EINVAL for a null array, B <= 0, an odd or
 * non-positive G, a non-positive res, n_theta, nx or ny, or a score volume
 * n_theta ny nx of 2^31 or more entries (slam_csm_work_size returns
 * SLAM_EINVAL for such a shape too). */
int64_t slam_csm_work_size(int32_t B, int32_t G, int32_t n_theta, int32_t ny, int32_t nx);
int slam_csm_batch(const double* pts, const int64_t* scan_off, const int32_t* src_scan, const int32_t* dst_scan,
                   const double* centre, const double* rot, int32_t B, double res, int32_t G, int32_t n_theta,
                   int32_t nx, int32_t ny, int32_t* out_best, int32_t* out_scores, void* work, void* stream);
/* Diagnostics: the score kernel gathers the table one byte per lane (1) or as
 * unaligned dwords, 4 adjacent shifts per lane summed as packed 16-bit pairs
 * (4, default; DESIGN.md section 3.5 has the A/B).  Per host thread; identical
 * results. */
int slam_csm_set_gather(int width);

/* ---- proximity loop-closure candidates (csrc/lcd_kernels.hip) --------------
 * The candidate search of src/loop_closure_detection.py:12-24
 * (detect_proximity): for every pose the nearest pose far enough along the
 * path, start[i] + np.argmin(cdist(xy, xy)[i, start[i]:]), without the N x N
 * matrix; new since ABI 103.
 *   poses     float64[N][3]  (x, y, theta; theta unused), finite
 *   start     int32[n_rows]  first admissible column of row i, 0 <= start[i]
 *             < N (the caller's np.searchsorted over the walked path length)
 *   n_rows    rows searched, n_rows <= N
 * For row i and column j: dx = x_i - x_j, dy = y_i - y_j, s = (dx dx) +
 * (dy dy) with three roundings (no FMA contraction), d(i, j) = sqrt(s)
 * correctly rounded.  out_j[i] is the SMALLEST j in [start[i], N) whose
 * d(i, j) is minimal and out_d[i] that d.  Ties are ties of the rounded
 * square roots, not of s: two different s may round to the same d, and the
 * earlier column wins even when its s is larger.  Partial results are merged
 * lexicographically on (d, j); no floating-point atomics: the result does not
 * depend on the launch shape.
 *   out_j     int32[n_rows]
 *   out_d     float64[n_rows]
 *   work      slam_lcd_work_size(N) BYTES, linear in N (at most 192 per pose)
 * SLAM_EINVAL for a null array, N <= 0, n_rows < 0 or n_rows > N
 * (slam_lcd_work_size: for N <= 0); n_rows == 0 succeeds without a launch. */
int64_t slam_lcd_work_size(int32_t N);
int slam_lcd_nearest_f64(const double* poses, int32_t N, const int32_t* start, int32_t n_rows, int32_t* out_j,
                         double* out_d, void* work, void* stream);

/* ---- binary-descriptor matching (csrc/desc_kernels.hip) ---------------------
 * The hot loop of src/loop_closure_detection.py:61-79 (matchify), which
 * detect_images_direct_similarity (:103) runs for every image pair: a
 * brute-force match of two images' ORB descriptors and the sum of the
 * n_matches best match distances; new since ABI 104.
 *   desc      uint8[D][32]  all descriptors, 16-byte aligned; image m holds the
 *             n_m >= 0 rows img_off[m] .. img_off[m + 1]
 *   img_off   int64[M + 1]  ascending, img_off[M] <= D
 *   qi, ti    int32[B]  query image (descriptors A) and train image (B) of pair b
 *   metric    0 hamming, 1 l2
 * hamming (cv2.BFMatcher(NORM_HAMMING, crossCheck=True).match(A, B), the
 * reference's approximate_match=False): d(a, b) = popcount(A[a] xor B[b]) in
 * 0..256; fwd[a] the smallest b with minimal d(a, .), bwd[b] the smallest a
 * with minimal d(., b); the matches are {(a, fwd[a]) : bwd[fwd[a]] == a}.
 * l2 (the exact search that the reference's default FLANN kd-tree
 * approximates: bytes as float32, one way, no cross-check): d(a, b) =
 * sum_c (A[a][c] - B[b][c])^2 as an integer, at most 2,080,800; the matches
 * are (a, fwd[a]) for every a; the distance OpenCV reports is sqrtf(d).
 * Both: the matches are ordered by (d, a) ascending (Python's stable
 * sorted(matches, key=distance) of a query-ordered list); count is their
 * number; the score is +inf when count < n_matches, otherwise the
 * left-to-right float64 sum over the first n_matches matches of d (hamming,
 * an exact integer) or of the float32 square root of d widened to float64
 * (l2; the fp64 root rounded to float32 is the same float for every possible
 * d, and distinct d have distinct roots).  An empty A or B gives count 0.
 * The first-index tie rules are believed to be BFMatcher's; parity with
 * OpenCV is unpinned.  Only integers decide the
 * outcome: every launch shape gives the same bits.
 *   out_score    float64[B]
 *   out_count    int32[B]
 *   out_matches  int32[B][n_matches][3] rows (a, b, d) of the first n_matches
 *                matches, or NULL; the rows of a pair with count < n_matches
 *                are filled with -1
 *   work         slam_desc_work_size(B, max_n, n_matches) BYTES (max_n: the
 *                most descriptors in one image); a pair's intermediates live
 *                in its workgroup's LDS, so the size is a fixed 256 today
 * Stream-ordered, graph-capturable, no host copies, nothing allocated.
 * SLAM_EINVAL for a null array (other than out_matches), a desc pointer not
 * 16-byte aligned, B < 0, M <= 0, an unknown metric or n_matches outside
 * 1..256; B == 0 succeeds without a launch.  What only the device can see is
 * checked there, pair by pair, like slam_icp_batch_f64's bounds: a pair that
 * names an image outside [0, M) (or whose offsets descend), or an image of
 * more than 4,096 descriptors, is not computed (out_score NaN, out_count -1,
 * rows -1) and raises a flag.  slam_desc_status synchronises `stream` and
 * reports the flag of every launch since the previous call, SLAM_OK,
 * SLAM_EINVAL (a bad image index) or SLAM_ETOOBIG, and clears it.
 * slam_desc_work_size returns SLAM_ETOOBIG for max_n > 4,096 itself. */
int64_t slam_desc_work_size(int32_t B, int32_t max_n, int32_t n_matches);
int slam_desc_match_batch(const uint8_t* desc, const int64_t* img_off, int32_t M, const int32_t* qi,
                          const int32_t* ti, int32_t B, int32_t metric, int32_t n_matches, double* out_score,
                          int32_t* out_count, int32_t* out_matches, void* work, void* stream);
int slam_desc_status(void* stream);
/* Diagnostics: how hamming finds bwd[b]: 0 (default) a second pass with the
 * roles swapped, 1 one pass with an LDS integer atomicMin of the packed key
 * d << 12 | a per distance (DESIGN.md section 3.7 has the A/B).  Per host
 * thread; identical results. */
int slam_desc_set_bwd(int mode);

/* ---- scan signatures (csrc/sig_kernels.hip) ---------------------------------
 * Loop-closure candidates from the scans themselves: a rotation-invariant
 * polar occupancy signature per scan and an all-pairs search over every
 * rotation.  The reference has no counterpart (its detectors need nearly right
 * poses or a camera); new since ABI 105.  The detector is for revisits in the
 * direction of travel at any rotation of the scan frame: a 270-degree scan
 * taken at a truly different heading sees other walls and is not matched.
 *
 * Parameters: S sectors, 8 <= S <= 128 and a multiple of 8; 32 rings;
 *   dirs      float64[S][2]  (cos, sin) of the sector centres (s + 0.5) 2 pi /
 *             S, evaluated by the caller (np.cos / np.sin, one scalar call each)
 *   edges2    float64[33]    squared ring edges (r_min + k dr)^2, nondecreasing
 * Signature of scan m (points pts[scan_off[m] .. scan_off[m + 1]) of the
 * packed float64[P][2] array of slam_icp_batch_f64): for every point (x, y),
 * r2 = (x x) + (y y) with three roundings (no FMA contraction); its ring is
 * the r with edges2[r] <= r2 < edges2[r + 1], and a point outside every ring
 * (or with a NaN coordinate) is dropped; its sector is the smallest s that
 * maximises (c_s x) + (s_s y), three roundings again (no atan2).
 *   sig       uint32[N][S]   bit r of sig[m][s] set when a point of scan m
 *             fell into (ring r, sector s)
 *   ring      uint8[N][32]   ring[m][r] = the number of sectors with bit r
 *             set; 16-byte aligned
 *   n_bits    int32[N]       their sum
 * A scan whose offsets descend or leave [0, P] gets the empty signature and
 * raises a flag (slam_sig_status).  SLAM_EINVAL for a null array, N < 0,
 * P < 0, a bad S or a misaligned ring; N == 0 succeeds without a launch. */
int slam_sig_build(const double* pts, const int64_t* scan_off, int32_t N, int64_t P, const double* dirs,
                   const double* edges2, int32_t S, uint32_t* sig, uint8_t* ring, int32_t* n_bits, void* stream);
/* Distance: d(i, j, k) = sum_s popcount(sig_i[s] xor sig_j[(s + k) mod S]);
 * d_ij is its minimum over k in [0, S) and k_ij the smallest k that attains
 * it (scan j's frame is turned by -2 pi k_ij / S against scan i's: the
 * rotation by -2 pi k_ij / S is the initial guess of icp(pc1 = scan j, pc2 =
 * scan i)).  For a row i < n_rows, scan j in [start[i], N) is a candidate iff
 * d_ij den <= num (n_i + n_j), compared in 64-bit integers.
 *   start      int32[n_rows]  0 <= start[i] <= N (N: no column); a start
 *              outside raises a flag (slam_sig_status) and its row is empty
 *   num, den   the threshold as a fraction, 0 <= num <= den, den >= 1
 *   K          1..16
 *   out_j, out_d, out_k  int32[n_rows][K]  the K smallest candidates by
 *              (d_ij, j) ascending: j, d_ij, k_ij; unused slots are -1
 *   out_count  int32[n_rows]  the number of candidates (may exceed K)
 *   work       slam_sig_work_size(N, S, K) BYTES, 8-byte aligned, linear in N
 *              (at most 16 column chunks of K partial entries per scan)
 * Exact screen: LB_ij = sum_r |ring_i[r] - ring_j[r]| <= d_ij (per ring,
 * popcount(a xor b) >= |popcount a - popcount b|, and a rotation keeps a
 * ring's popcount), so a pair with LB_ij den > num (n_i + n_j) is skipped
 * without changing any output.  Only integers decide anything: every launch
 * shape gives the same bits.  Stream-ordered, graph-capturable, no host
 * copies, nothing allocated.  SLAM_EINVAL for a null array, N <= 0, a bad S,
 * K or threshold, n_rows outside [0, N] or a misaligned ring / work;
 * n_rows == 0 succeeds without a launch.  slam_sig_status synchronises
 * `stream`, reports the flags of every launch since the previous call
 * (SLAM_OK or SLAM_EINVAL) and clears them. */
int64_t slam_sig_work_size(int32_t N, int32_t S, int32_t K);
int slam_sig_match(const uint32_t* sig, const uint8_t* ring, const int32_t* n_bits, int32_t N, int32_t S,
                   const int32_t* start, int32_t n_rows, int32_t num, int32_t den, int32_t K, int32_t* out_j,
                   int32_t* out_d, int32_t* out_k, int32_t* out_count, void* work, void* stream);
int slam_sig_status(void* stream);
/* Diagnostics: the ring-count screen on (1, default) or off (0: every pair is
 * evaluated).  Per host thread; identical results. */
int slam_sig_set_screen(int on);

/* ---- pairwise consistency of loop closures (csrc/pcm_kernels.hip) -------------
 * Verifies the loop closures against each other before they reach an
 * optimiser (pairwise consistent measurement set selection): two closures are
 * consistent when the cycle they form with the chain of poses closes to within
 * the chain's drift, and a large pairwise consistent set is kept.  The reference
 * has no counterpart; new since ABI 106.
 *
 * An SE(2) element is four doubles (c, s, x, y).  Every operation below is
 * individually rounded (no FMA contraction):
 *   mul(A, B): c = A.c B.c - A.s B.s          s = A.s B.c + A.c B.s
 *              x = (A.c B.x - A.s B.y) + A.x  y = (A.s B.x + A.c B.y) + A.y
 *   inv(A):    c = A.c   s = -A.s   x = -(A.c A.x + A.s A.y)   y = A.s A.x - A.c A.y
 *   X      float64[N][4]  the chain poses, (cos, sin) evaluated by the caller
 *          (np.cos / np.sin, one scalar call each): no transcendental here
 *   a, b   int32[L]       closure l measures X_b = X_a Z ("relative" convention)
 *   Z      float64[L][4]
 * Per closure: V = X[a], D = mul(mul(V, Z), inv(X[b])), Di = inv(D), U =
 * mul(inv(V), D).  Per unordered pair l < m: E = mul(mul(U_l, Di_m), V_l) (the
 * cycle a_l -> b_l -> b_m -> a_m -> a_l in a_l's frame), n = |a_l - a_m| +
 * |b_l - b_m|, dt = E.x E.x + E.y E.y, dr = E.s E.s + (1 - E.c)(1 - E.c); the
 * pair is consistent iff dt <= trans_tol^2 + (trans_drift^2) n and dr <=
 * rot_tol^2 + (rot_drift^2) n (a floor plus random-walk growth, in variance
 * form).  A NaN compares false: such a closure is consistent with nothing.
 *   out_adj  uint32[L][W], W = ceil(L / 32): bit m of row l is bit m & 31 of
 *            word m >> 5; bits (l, m) and (m, l) both come from the pair
 *            evaluated as (min, max), the diagonal and the bits past L are 0
 *   out_deg  int32[L]      the rows' popcounts
 *   work     slam_pcm_work_size(L) BYTES, 8-byte aligned (96 per closure)
 * An a or b outside [0, N) raises a flag (slam_pcm_status); it is never read
 * through and its row and column are empty.
 *
 * slam_pcm_select is a min-degree peel: with every closure alive, repeat: take
 * the alive closure of the lowest degree, on ties the HIGHEST index; if its
 * degree is the number of the others alive, they are a clique: stop; otherwise
 * remove it (out_order = the step, from 0) and decrement its alive neighbours.
 *   out_order  int32[L]   the removal step, -1 for a closure never removed
 *   out_keep   uint8[L]   1 for the closures left, all 0 when fewer than
 *              min_size are left
 *   out_steps  int32[1]   the number of removals
 * deg is only read.  The result is A maximal consistent set, not the maximum
 * one.  One workgroup; a step costs one block minimum and one bit row.
 *
 * Stream-ordered, graph-capturable, no host copies, nothing allocated.
 * SLAM_EINVAL for a null array, L < 0, N <= 0, min_size < 0, a negative
 * tolerance or a misaligned work; SLAM_ETOOBIG for L > 65,536 (a 512 MB
 * matrix; index and degree are 16-bit fields of the peel's keys); L == 0
 * succeeds without a launch.  slam_pcm_status synchronises `stream`, reports
 * the flag of every launch since the previous call (SLAM_OK or SLAM_EINVAL)
 * and clears it. */
int64_t slam_pcm_work_size(int32_t L);
int slam_pcm_adjacency_f64(const double* X, int32_t N, const int32_t* a, const int32_t* b, const double* Z, int32_t L,
                           double trans_tol, double trans_drift, double rot_tol, double rot_drift, uint32_t* out_adj,
                           int32_t* out_deg, void* work, void* stream);
int slam_pcm_select(const uint32_t* adj, const int32_t* deg, int32_t L, int32_t min_size, int32_t* out_order,
                    uint8_t* out_keep, int32_t* out_steps, void* stream);
int slam_pcm_status(void* stream);
/* Diagnostics: closures per thread of the peel's one workgroup: 0 (default)
 * the smallest of 1, 4, 16, 64 that covers L, or one of them as the least
 * (four instantiations of one kernel).  Per host thread; identical results. */
int slam_pcm_set_peel_slots(int slots);

/* ---- point-to-line refinement of ICP edges (csrc/plicp_kernels.hip) -----------
 * Refines a scan pair's transform with a gated point-to-line metric
 * (Gauss-Newton on the distance to the matched point's tangent line), which
 * does not pull along the walls as the point-to-point metric of
 * slam_icp_batch_f64 does.  The reference has no counterpart; new since ABI
 * 107.  Scans are the packed layout of slam_icp_batch_f64: pts float64[P][2]
 * (16-byte aligned), scan_off int64[S + 1], the points of a scan in beam order.
 * All arithmetic is fp64 and every product and sum below is rounded on its own
 * (no FMA contraction), written with its parentheses; coordinates are finite.
 *
 * Normals, once per scan.  K neighbours per side (>= 1), rho2 the squared
 * support radius (the caller's rho * rho), ctol the corner tolerance.  For
 * point j of a scan of n points Q[0..n), with d2(a, b) = ((Qa.x - Qb.x)^2) +
 * ((Qa.y - Qb.y)^2):
 *   support  l = j; while l > 0, j - l < K and d2(l - 1, j) <= rho2: --l.
 *            r = j; while r < n - 1, r - j < K and d2(r + 1, j) <= rho2: ++r.
 *            r - l < 2: no normal.
 *   tangent  t = Q[r] - Q[l], L2 = (t.x t.x) + (t.y t.y); L2 not > 0 or not
 *            finite: no normal.  L = sqrt(L2), n = (-t.y / L, t.x / L) (IEEE
 *            square root and division).
 *   corner   off = (n.x (Qj.x - Ql.x)) + (n.y (Qj.y - Ql.y)); |off| > ctol: no
 *            normal.
 *   out_normals  float64[P][2], (0, 0) for none; 16-byte aligned.  Points that
 *            belong to no scan get (0, 0) too (the array is zeroed first).
 * A scan whose offsets descend or leave [0, P] gets no normals and raises a
 * flag (slam_plicp_status).  SLAM_EINVAL for a null array, S < 0, P < 0,
 * K < 1, a negative or non-finite rho2 or ctol or a misaligned array; S == 0
 * succeeds without a launch. */
int slam_plicp_normals_f64(const double* pts, const int64_t* scan_off, int32_t S, int64_t P, int32_t K, double rho2,
                           double ctol, double* out_normals, void* stream);
/* Refinement of B pairs, one workgroup per pair, every iteration on chip.
 *   src_scan, dst_scan  int32[B]  scan indices, as slam_icp_batch_f64
 *   init       float64[B][9]  T maps source points into the destination
 *              frame; its bottom row is taken as 0 0 1
 *   normals    float64[P][2]  slam_plicp_normals_f64's output for these scans
 *   max_dist2  the squared correspondence gate; min_inliers; max_iters >= 1;
 *   eps_t, eps_r  the stopping steps; pivot_tol (1e-9 is the usual value)
 *   max_n1     an upper bound of the source scans' sizes, <= 8,192
 * Per iteration, from T:
 *   transform  x' = ((T00 x) + (T01 y)) + T02, y' = ((T10 x) + (T11 y)) + T12
 *   match      j* the smallest j that minimises ((x' - qx)^2) + ((y' - qy)^2)
 *              over the destination scan
 *   gate       the point is an inlier iff that minimum is <= max_dist2; m
 *              inliers
 *   rows       ex = x' - qx, ey = y' - qy.  An inlier whose match has a normal
 *              (nx, ny): a = (nx, ny, (ny x') - (nx y')), r = (nx ex) + (ny ey).
 *              One whose match has none, two rows (the point-to-point
 *              fallback): a = (1, 0, -y'), r = ex and a = (0, 1, x'), r = ey.
 *   sums       H = sum a a^T (six sums), g = sum a r, e = sum r r over all
 *              rows, in the implementation's own order: fixed (no
 *              floating-point atomics), so a pair gives the same bits in any
 *              batch, at any slot
 *   err = e / m;  h = (H00 + H11) / 2, q = sqrt(max((h h) - ((H00 H11) - (H01
 *              H01)), 0)), obs = (h - q) / (h + q): near 0 in a corridor, near
 *              1 in a room
 *   too few    m < min_inliers: stop, status TOO_FEW, T unchanged
 *   solve      H delta = -g by LDL^T in the order (x, y, theta): d0 = H00, l10 =
 *              H01 / d0, l20 = H02 / d0, d1 = H11 - (l10 H01), u = H12 - (l20
 *              H01), l21 = u / d1, d2 = (H22 - (l20 H02)) - (l21 u); z0 = -g0,
 *              z1 = -g1 - (l10 z0), z2 = (-g2 - (l20 z0)) - (l21 z1); dth = z2 /
 *              d2, dy = (z1 / d1) - (l21 dth), dx = ((z0 / d0) - (l10 dy)) - (l20
 *              dth).  A pivot d_k that is not finite or <= pivot_tol H_kk: stop,
 *              status DEGENERATE, T unchanged
 *   update     c = cos dth, s = sin dth, T <- [[c, -s, dx], [s, c, dy], [0, 0,
 *              1]] T with plain products and sums: T00 = (c T00) - (s T10), T02
 *              = ((c T02) - (s T12)) + dx, T10 = (s T00) + (c T10), T12 = ((s
 *              T02) + (c T12)) + dy, the middle column like the first; ++it
 *   stop       |dx| < eps_t, |dy| < eps_t and |dth| < eps_r: CONVERGED;
 *              otherwise it == max_iters: MAX_ITERS (its transform is usable)
 * Outputs per pair: out_tf[9]; out_iters; out_status 0 CONVERGED, 1
 * MAX_ITERS, 2 DEGENERATE, 3 TOO_FEW; out_err, out_obs and out_inliers are
 * those of the LAST LINEARISATION, that is of the transform before the final
 * step (for TOO_FEW and DEGENERATE: of the linearisation that stopped; err is
 * NaN when it had no inlier).  out_match int32[B][match_stride], NULL allowed:
 * j* of the last linearisation per source point, -1 for an outlier and past
 * the scan's end; match_stride >= max_n1.
 * What only the device can see is checked there, pair by pair: a pair that
 * names a scan outside [0, S), whose offsets descend or leave [0, P], or whose
 * source scan exceeds max_n1 is not computed (out_status -1, out_tf = init,
 * err and obs NaN, match -1) and raises a flag.  slam_plicp_status
 * synchronises `stream`, reports the flags of every launch of both entry
 * points since the previous call (SLAM_OK or SLAM_EINVAL) and clears them.
 * Stream-ordered, graph-capturable, no host copies, nothing allocated.
 * SLAM_EINVAL for a null array (other than out_match), B < 0, max_iters < 1,
 * a negative or non-finite max_dist2, eps_t, eps_r or pivot_tol, a stride
 * below max_n1 or a misaligned array; SLAM_ETOOBIG for max_n1 > 8,192 (the
 * limit of slam_icp_batch_f64); B == 0 succeeds without a launch. */
int slam_plicp_batch_f64(const double* pts, const int64_t* scan_off, int32_t S, int64_t P, const double* normals,
                         const int32_t* src_scan, const int32_t* dst_scan, const double* init, int32_t B,
                         double max_dist2, int32_t min_inliers, int32_t max_iters, double eps_t, double eps_r,
                         double pivot_tol, int32_t max_n1, double* out_tf, double* out_err, double* out_obs,
                         int32_t* out_inliers, int32_t* out_iters, int32_t* out_status, int32_t* out_match,
                         int32_t match_stride, void* stream);
int slam_plicp_status(void* stream);

/* ---- verification of an edge by scan visibility (csrc/vis_kernels.hip) ---------
 * Says, for one edge icp(pc1 = src, pc2 = dst) -> T on its own, whether T is
 * believable: the points of one scan, mapped into the other scan's frame, must
 * lie on the surface that scan measured at their bearing and not in front of
 * it, where that scan saw free space.  The reference has no counterpart; new
 * since ABI 108.  Scans are the packed layout of slam_icp_batch_f64.  All
 * arithmetic is fp64, every written parenthesis below is one rounding (no FMA
 * contraction), sqrt is the IEEE square root.  The scans keep no record of
 * beams without a return, so a direction without a point is "unknown".
 *
 *   dirs      float64[S][2]  sector centres (cos, sin)((k + 0.5) 2 pi / S), made
 *             by the caller; 3 <= S <= 1024
 *   sector    of a point (x, y): the first maximum over k = 0..S-1 of
 *             (c_k x) + (s_k y) (a comparison with NaN is false: sector 0)
 *   table     of a scan: R2[k] = the minimum of r2 = (x x) + (y y) over the
 *             scan's points in sector k; +inf for an empty sector; a point
 *             whose r2 is not finite takes no part.  A minimum of non-negative
 *             doubles is exact and order-free.
 * slam_vis_tables_f64 writes out_r2 float64[n_scans][S], one workgroup per
 * scan.  A scan whose offsets descend or leave [0, P] keeps a row of +inf and
 * raises a flag.
 *
 * One direction of an edge: the points p of scan A through a transform M
 * against scan B's table, window W >= 0 (2 W + 1 <= S), margin >= 0:
 *   q         qx = ((M00 x) + (M01 y)) + M02, qy = ((M10 x) + (M11 y)) + M12
 *   rq = sqrt((qx qx) + (qy qy)), k the sector of q
 *   entries   e_w = R2_B[(k + w) mod S], w = -W..W; seen iff finite, then
 *             re_w = sqrt(e_w)
 *   agrees    |re_w - rq| <= margin for some seen entry
 *   conflicts it does not agree, all 2 W + 1 entries are seen and
 *             rq + margin < min_w re_w
 *   unknown   otherwise (rq not finite: always)
 * An edge: direction 0 maps src's points through T (bottom row taken as 0 0 1)
 * against dst's table; direction 1 maps dst's points against src's table
 * through the rigid inverse, rotation the transpose of T's 2x2 block,
 * translation (-((T00 tx) + (T10 ty)), -((T01 tx) + (T11 ty))).
 *   out_counts int32[B][6]  (agree0, conflict0, n0, agree1, conflict1, n1), n_d
 *             the number of points mapped in direction d
 * Counts are integer sums of per-wave popcounts: the same for any launch
 * shape.  An edge that names a scan outside [0, n_scans), or one whose offsets
 * descend or leave [0, P], is not computed: its six counts are -1 and a flag
 * is raised; the other edges of the launch are unaffected.  slam_vis_status
 * synchronises `stream`, reports the flags of every launch of both entry
 * points since the previous call (SLAM_OK or SLAM_EINVAL) and clears them.
 * The verdict (which shares of agreeing and conflicting points pass) is the
 * caller's: slamhip.vis.VisParams.passes.
 * Stream-ordered, graph-capturable, no host copies, nothing allocated.
 * SLAM_EINVAL, before any launch, for a null array, S outside 3..1024, W < 0
 * or 2 W + 1 > S, a negative or non-finite margin, negative sizes or
 * misaligned points; B == 0 and n_scans == 0 succeed without a launch. */
int slam_vis_tables_f64(const double* pts, const int64_t* scan_off, int32_t n_scans, int64_t P, const double* dirs,
                        int32_t S, double* out_r2, void* stream);
int slam_vis_check_f64(const double* pts, const int64_t* scan_off, int32_t n_scans, int64_t P, const double* dirs,
                       int32_t S, const double* tables, const int32_t* src, const int32_t* dst, const double* tf,
                       int32_t B, double margin, int32_t W, int32_t* out_counts, void* stream);
int slam_vis_status(void* stream);

/* ---- localisation in a finished occupancy grid (csrc/loc_kernels.hip) ----------
 * Where a scan lies in the map that produce_occupancy_grid made: the int8 grid
 * (H, W), row = y, its origin (min_x, min_y) and its cell width cw.  The
 * reference has no counterpart; new since ABI 109.  Scans are the packed layout
 * of slam_icp_batch_f64.  tests/loc_ref.py restates all three definitions.
 *
 * Field.  Cell (r, c) is occupied iff grid[r][c] > occ_min (grid_mle's rule at
 * 0); d_cap in 1..255 cells:
 *   F[r][c] = min(d_cap^2, min over occupied (r', c') of (r - r')^2 + (c - c')^2)
 * as uint16; d_cap^2 everywhere without an occupied cell in reach.  Integers
 * only: exact.  work: slam_loc_field_work_size(H, W) BYTES.  SLAM_EINVAL for a
 * null array, H or W <= 0, H > 65,535, d_cap outside 1..255, occ_min outside
 * int8. */
int64_t slam_loc_field_work_size(int32_t H, int32_t W);
int slam_loc_field(const int8_t* grid, int32_t H, int32_t W, int32_t occ_min, int32_t d_cap, uint16_t* out_field,
                   void* work, void* stream);
/* Window search of B queries against the one field.
 *   q_scan    int32[B]  the query's scan
 *   centre    float64[B][3]  (theta0, x0, y0) in the map frame
 *   rot       float64[B][n_theta][2]  (cos, sin) of theta_k = theta0 +
 *             (k - n_theta / 2) d_theta, evaluated by the caller as for
 *             slam_csm_batch
 *   nx, ny, step   shift window: (i - nx / 2) step cells in x, (j - ny / 2)
 *             step cells in y, step >= 1
 * A point (px, py) of the scan maps to gx = (c px - s py) + x0, gy = (s px +
 * c py) + y0 (every operation rounded on its own), its cell is cx = floor((gx -
 * min_x) / cw), cy = floor((gy - min_y) / cw) (true fp64 division).  Cost
 * C[k][j][i] = sum over the scan's points of F[cy + (j - ny / 2) step][cx +
 * (i - nx / 2) step], a cell outside the grid (or beyond int32) adding d_cap^2.
 * Only integers are summed: the result does not depend on summation order or
 * launch shape.
 *   max_n       the largest queried scan; max_n d_cap^2 >= 2^31 is refused
 *   out_best    int32[B][4]  minimum cost, then k, j, i of the minimum with
 *               the smallest flat index (k ny + j) nx + i
 *   out_costs   int32[B][n_theta][ny][nx] the whole volume, or NULL
 *   work        slam_loc_search_work_size(B, H, W, n_theta, ny, nx, step) BYTES
 * The caller assembles the pose from theta_k, x0 + (i - nx / 2) step cw and
 * y0 + (j - ny / 2) step cw.  A query that names a scan outside [0, S), one
 * whose offsets descend or leave [0, P], or one of more than max_n points is
 * not computed: its out_best row is -1 (its costs are not written) and a flag
 * is raised; slam_loc_status synchronises `stream`, reports the flags of every
 * launch of the search and the refinement since the previous call (SLAM_OK or
 * SLAM_EINVAL) and clears them.  SLAM_EINVAL, before any launch, for a null
 * array, B <= 0, a non-positive H, W, cw, n_theta, nx, ny or step, d_cap
 * outside 1..255, a cost volume n_theta ny nx of 2^31 or more entries, a
 * bordered table (H + 2 ny step) (W + 2 nx step) of 2^31 or more cells, or
 * max_n d_cap^2 >= 2^31 (slam_loc_search_work_size returns SLAM_EINVAL for
 * such a shape too). */
int64_t slam_loc_search_work_size(int32_t B, int32_t H, int32_t W, int32_t n_theta, int32_t ny, int32_t nx,
                                  int32_t step);
int slam_loc_search(const uint16_t* field, int32_t H, int32_t W, double min_x, double min_y, double cell_width,
                    int32_t d_cap, const double* pts, const int64_t* scan_off, int32_t S, int64_t P,
                    const int32_t* q_scan, const double* centre, const double* rot, int32_t B, int32_t max_n,
                    int32_t n_theta, int32_t nx, int32_t ny, int32_t step, int32_t* out_best, int32_t* out_costs,
                    void* work, void* stream);
/* Diagnostics: the search gathers a table of 2-byte entries (2, default) or,
 * when d_cap <= 15, of 1-byte entries (1; DESIGN.md section 3.12 has the A/B).
 * Per host thread; identical results. */
int slam_loc_set_table(int width);
/* Sub-cell refinement: Gauss-Newton on the field in metres from init[b] =
 * (theta, x, y), one pose per query.  D[r][c] = sqrt(F[r][c]) cw (IEEE square
 * root of the integer, one product), sampled at cell centres, bilinear between
 * them.  Per iteration c = cos(theta), s = sin(theta) (the device's; the only
 * values that may differ from the restatement's in the last place), and per
 * point (every written parenthesis one rounding, no FMA contraction):
 *   gx = ((c px) - (s py)) + x,  gy = ((s px) + (c py)) + y
 *   u = ((gx - min_x) / cw) - 0.5,  v = ((gy - min_y) / cw) - 0.5
 *   i0 = floor(u), j0 = floor(v), a = u - i0, b = v - j0
 *   D00 = D[j0][i0], D10 = D[j0][i0 + 1], D01 = D[j0 + 1][i0], D11 = D[j0 + 1][i0 + 1]
 *   r  = ((1 - b) (((1 - a) D00) + (a D10))) + (b (((1 - a) D01) + (a D11)))
 *   jx = (((1 - b) (D10 - D00)) + (b (D11 - D01))) / cw
 *   jy = (((1 - a) (D01 - D00)) + (a (D11 - D10))) / cw
 *   jt = (jx ((-s px) - (c py))) + (jy ((c px) - (s py)))
 * A point is left out when one of its four cells is outside the grid (i0 outside
 * 0..W-2 or j0 outside 0..H-2, tested in fp64) or all four F equal d_cap^2.  The
 * m inliers' rows J = (jx, jy, jt) give H = sum J J^T, g = sum J r, e = sum r r,
 * plain fp64 sums in this order: thread t of the 256 adds its points t, t + 256,
 * ... in ascending order; the 64 threads of a wave are added by common.hpp's
 * wave_sum tree, the four waves in ascending order.  The launch shape is fixed,
 * so the order is.  rms = sqrt(e / m).
 *   status 3  m == 0 or m < min_inlier_frac n (n the scan's points): stop
 *   status 2  LDL^T pivots d_k of H as in slam_plicp_batch_f64: a pivot that is
 *             not finite or d_k <= pivot_tol H_kk: stop
 *   otherwise (dx, dy, dth) = -H^-1 g by that factorisation; x += dx, y += dy,
 *             theta += dth, iters += 1
 *   status 0  sqrt((dx dx) + (dy dy)) < eps_t and |dth| < eps_r
 *   status 1  iters == max_iters
 * Outputs per query: out_pose (theta, x, y), out_rms and out_inliers of the last
 * linearisation, out_iters, out_status.  A query outside its bounds (as for the
 * search) keeps its init pose, rms NaN, status -1, and raises the flag.
 * SLAM_EINVAL for a null array, a negative size, max_iters < 1, a negative or
 * non-finite tolerance, min_inlier_frac above 1, a bad grid shape or d_cap;
 * B == 0 succeeds without a launch. */
int slam_loc_refine_f64(const uint16_t* field, int32_t H, int32_t W, double min_x, double min_y, double cell_width,
                        int32_t d_cap, const double* pts, const int64_t* scan_off, int32_t S, int64_t P,
                        const int32_t* q_scan, const double* init, int32_t B, int32_t max_n, int32_t max_iters,
                        double eps_t, double eps_r, double min_inlier_frac, double pivot_tol, double* out_pose,
                        double* out_rms, int32_t* out_inliers, int32_t* out_iters, int32_t* out_status, void* stream);
int slam_loc_status(void* stream);

/* Diagnostics (kernel-shape sweeps; not needed by callers). */
int slam_icp_num_instances(void);
int slam_icp_instance_shape(int i, int* block, int* qpt);
int slam_icp_force_instance(int i);
int slam_icp_selected_instance(int max_n1);
/* NN search mode: 0 exact fp64 scan, 1 fp32 screen (all chunks), 2 fp32
 * screen with exact pruning (per-lane windows + sub-chunk boxes, default);
 * identical results. */
int slam_icp_set_screen(int mode);
/* Phased scheduling of slam_icp_batch_f64 for batches of >= min_pairs pairs:
 * every pair runs probe_iters iterations, then the unfinished ones resume in
 * order of their last error change (slowest-converging first), so the long
 * tail of iteration counts does not start late.  probe_iters = 0: one launch;
 * -1 (default): automatic — 3, or 4 for batches of 2,048-4,095 pairs and 2
 * for 4,096-8,192.
 * Defaults (-1, 1024).  Results are identical either way. */
int slam_icp_set_schedule(int probe_iters, int min_pairs);
/* Phase 2 of the scheduler starts the (at most) `heads` pairs the probe keyed
 * slowest (one per 16 pairs at most) first, on CU-exclusive 512-thread
 * workgroups; the rest runs beside them on a library-owned second stream,
 * joined back before the call's work ends: the strong-scaling tail.  Batches
 * below 4,096 pairs only (larger shards keep every CU for the bulk).  Sums
 * are order-free (exact on fixed grids), so results are bit-identical to the
 * single launch.  0 = off; default 64. */
int slam_icp_set_schedule_heads(int heads);
/* The first `gangs` of those head pairs run as gangs of `parts` workgroups
 * (2..17) each: a pair's 64-query groups are dealt over the parts, which sit on
 * one XCD, hold one CU each, and exchange their exact partial sums every
 * iteration through a stream-ordered workspace (data-tagged 8-byte granules,
 * agent-scope write-through stores, bounded polling).  parts = 0: teams, one
 * workgroup per 64-query group (pairs up to 2,048 points), the group's search
 * split over the workgroup's four waves (latency mode).  Results are
 * bit-identical to the one-workgroup kernels.  gangs = 0: off; defaults
 * (24, 4).  SLAM_EINVAL for gangs < 0, parts 1, < 0 or > 17. */
int slam_icp_set_schedule_gangs(int gangs, int parts);
/* Wide tier: the `pairs` slowest-keyed pairs (taken before the gangs) run on
 * one workgroup per 64-query group (pairs up to 2,048 points) whose NW waves
 * split a brute-force fp32 screen by candidate slices (no pruning, so no
 * outlier group sets the iteration time); the groups exchange their exact
 * partial sums every iteration like the gangs.  Workgroups request 1/share of
 * a CU's LDS (1: CU-exclusive).  Bit-identical results; 0 = off. */
int slam_icp_set_schedule_wide(int pairs, int share);
/* Bulk gangs: batches of fewer than `below_pairs` pairs run the bulk of both
 * scheduler phases as gangs of `parts` (2 or 3) workgroups with the ordinary
 * LDS footprint — half (a third) of a pair's iteration latency when whole
 * pairs cannot fill the GPU (strong-scaling shards).  Bit-identical results.
 * below_pairs = 0: off. */
int slam_icp_set_bulk_gangs(int below_pairs, int parts);
/* Diagnostics: the scheduler can save a paused pair's search state (last match
 * and clearance per query, 8 B, and the pending motion bound) so its phase-2
 * iteration starts warm (1; a transient workspace of 8 B per query — measured
 * no faster on C3, round 4); 0 (default) resumes cold.  Results are identical. */
int slam_icp_set_schedule_warm(int on);
/* Gang parts that waited longer than the gang wait for a partner since the
 * last call (read-and-clear; synchronises the device): 4 ms at a pair's first
 * exchange of a launch (a partner that is not resident by then, e.g. CUs held
 * by another process), 0.2 s later on.  Such a part stops at once without
 * writing and marks its next exchange so that partners already past this one
 * stop there too; a first-exchange timeout also stops every other pair of the
 * same launch at its first exchange (one wait per launch, not per pair);
 * after phase 2 the scheduler re-runs every exchange-tier pair
 * that did not finish on one workgroup from its saved state, so the results
 * stay valid (and bit-identical): this count is a warning, not an error.
 * Scheduler order is a stable sort (deterministic). */
int slam_icp_gang_timeouts(void);
/* Diagnostics: the gang wait in s_memrealtime ticks (100 MHz); 0 = default.
 * Tiny values force timeouts, exercising the repair path (the first
 * exchange's wait is the smaller of this and slam_icp_set_gang_first_wait's). */
int slam_icp_set_gang_wait(uint32_t ticks);
/* Diagnostics: the first exchange's wait in ticks; 0 = default (4 ms). */
int slam_icp_set_gang_first_wait(uint32_t ticks);
/* Diagnostics: `workgroups` workgroups that each hold a whole CU's LDS and
 * spin for `ticks` (<= 1 s) on `stream` — a stand-in for another process
 * occupying CUs while a batch runs. */
int slam_icp_diag_occupy(int workgroups, uint32_t ticks, void* stream);
/* Diagnostics: phase 2's visiting order of B pairs from their phase-1
 * out_iters (> 0: finished) and keys (last |dE|), by the scheduler's stable
 * bucket sort (device arrays; order[] receives B pair indices). */
int slam_icp_sched_sort(const int32_t* iters, const float* key, int32_t B, float thresh, int32_t* order,
                        void* stream);
/* Diagnostics: batches of <= 8,192 pairs sort at the phase boundary on one
 * workgroup (1, default; slam_icp_sched_sort uses it at those sizes too) or
 * with the three-kernel sort (0).  The order is the same. */
int slam_icp_set_sched_sort_one(int on);
/* Diagnostics: batches of fewer than `pairs` pairs get the scheduler's tail
 * tiers (heads, gangs, wide); 0 restores the default (4,096). */
int slam_icp_set_tier_limit(int pairs);
/* Diagnostics: the angle pre-tier — batches of up to 8,192 pairs run up to
 * `max_pairs` pairs whose initial transform turns by more than `thresh_rad`
 * on a tier of their own from the start (slam_icp_set_angle_tier_kind),
 * beside the two-phase schedule of the others (0: off).  Results are
 * bit-identical. */
int slam_icp_set_angle_tier(int max_pairs, float thresh_rad);
/* Diagnostics: the angle pre-tier's kind, 0 the wide tier, 2 / 3 / 4 / 6 bulk
 * gangs of that many ordinary workgroups per pair. */
int slam_icp_set_angle_tier_kind(int kind);
/* Diagnostics: with a gang pre-tier (kind 2 / 3), its first wide_pairs
 * turning pairs (the largest turns) run on wide workgroups, `share` per CU,
 * the rest on the gangs (0: none).  Bit-identical. */
int slam_icp_set_angle_tier_mix(int wide_pairs, int share);
/* Diagnostics: query groups per wide-tier workgroup: 1 (8 waves, `share`
 * workgroups per CU) or 2 (16 waves, one workgroup per CU; a 1081-point pair
 * on 9 workgroups).  Bit-identical. */
int slam_icp_set_wide_groups(int groups);
/* The scheduler's automatic tier profile by batch size (1, default; DESIGN.md
 * section 6): below 2,048 pairs up to 40 turning pre-tier pairs, below 4,096
 * up to 64, on wide workgroups of two query groups (one per CU); 4,096 - 8,192
 * pairs up to 96 pre-tier pairs on gangs of 4 plus 64 phase-2 heads, the
 * first 24 as gangs of 4; larger batches no tiers.  0: the explicit settings;
 * any of the tier setters above selects them, 1 restores their defaults too. */
int slam_icp_set_schedule_auto(int on);
/* The drain tier of phased batches: once every pair of phase 2's bulk launch
 * has started and at most `pairs` still run, each of them pauses at the end of
 * its iteration and they finish on wide workgroups (two query groups, one per
 * CU), from their paused state, bit-identical.  -1: the default (24 for
 * batches up to 8,192 pairs, off above), 0: off, at most 64 (more than
 * 256 / parts pairs cannot all be resident: their exchanges time out and the
 * repair launch finishes them). */
int slam_icp_set_drain(int pairs);
/* Diagnostics: the XCD-aware pair map of launches in stream order: runs of
 * `run` consecutive pairs per XCD (default 16, so consecutive pairs share
 * their common scan through one L2 while the runs rotate over the XCDs),
 * 0 the identity, -1 the default. */
int slam_icp_set_xcd_map(int run);
int slam_gn_set_stamps(void* dev_buf);
/* GN linear solver (per host thread): 0 auto (block cyclic reduction when the
 * band allows it), 1 band Cholesky, 2 block cyclic reduction (falls back to 1
 * if the band is too wide).  A bordered plan (slam_gn_iteration_bordered_f64)
 * needs the cyclic-reduction solver: with mode 1, or a band too wide for it,
 * that entry point returns SLAM_EINVAL; slamhip.gn plans without a border
 * while mode 1 is set (slam_gn_get_solver). */
int slam_gn_set_solver(int mode);
int slam_gn_get_solver(void);
/* Block rows of the cyclic-reduction solver for (nv, W), 0 = not applicable. */
int slam_gn_bcr_block_rows(int32_t nv, int32_t W);
/* Diagnostics: per-phase s_memtime totals of workgroup 0 into a device buffer of
 * >= 160 uint64 (wave 0's sub-phases in [0, 16), every wave's phase totals in
 * [16 + 8 * wave, 24 + 8 * wave), the pruned search's group iterations, live and
 * visited sub-chunks by active-lane bucket in [96, 120)); NULL turns stamping off. */
int slam_icp_set_stamps(void* dev_buf);
/* Count candidate-distance evaluations performed (all lanes) into a device
 * uint64 (atomic add per wave); NULL turns counting off.  Stamps and the
 * counter run in a separate diagnostics build of the pruned batch kernel
 * (NN mode 2, slam_icp_batch_f64 only); the product kernels carry neither. */
int slam_icp_set_eval_counter(void* dev_u64);
/* Diagnostics: the per-pair phase timeline of slam_icp_batch_f64 into a device
 * buffer of B x 2 x 4 uint64 — per pair and scheduler phase the
 * s_memrealtime (100 MHz) at which its workgroup (part 0) started and ended
 * and where it ran (XCC << 32 | HW_ID); NULL turns it off. */
int slam_icp_set_trace(void* dev_buf);

#ifdef __cplusplus
}
#endif
#endif /* SLAMHIP_H */

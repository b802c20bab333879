/*
 * sfmcore.h -- C-ABI of libsfmcore.so, the MI355X (gfx950) numerical core
 * that replaces the reference's hot path
 *   EstimateFundamentalMatrix -> GetInliersRANSAC -> LinearTriangulation
 *   -> BundleAdjustment       (pvrohin/Structure-from-Motion-, "Phase 1/").
 *
 * Plain C types only: caller-owned, row-major, C-contiguous host buffers,
 * int return codes (0 = OK, < 0 = error; message via sfm_last_error()).
 * No C++ exception crosses this line.  Every entry point is reentrant: each
 * host thread gets its own HIP stream and scratch buffers per device.
 *
 * The Python drop-in modules in structure-from-motion-_amd/ bind these with
 * ctypes (_sfmcore.py); INTEGRATION.md shows the binding.
 */
#ifndef SFMCORE_H
#define SFMCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFM_ABI_VERSION 1

enum {
    SFM_OK = 0,
    SFM_ERR_ARG = -1,     /* bad argument (shape, null pointer, range)   */
    SFM_ERR_HIP = -2,     /* HIP runtime error                           */
    SFM_ERR_NOMEM = -3,   /* device allocation failed                    */
    SFM_ERR_SOLVE = -4,   /* reduced camera system not positive definite */
    SFM_ERR_COMM = -5,    /* RCCL error                                  */
    SFM_ERR_CAPACITY = -6, /* a result exceeds the caller's output arrays */
    SFM_ERR_NUMERIC = -7   /* an iterate left the range a stage defines    */
};

int sfm_version(void);
/* last error message of the calling thread ("" if none) */
const char *sfm_last_error(void);
int sfm_device_count(void);
/* per-call phase timings of the calling thread's last call (ms):
 * [0] host->device upload, [1] kernels, [2] device->host download,
 * [3] kernel-only time of the dominant kernel.  Returns the count written. */
int sfm_last_timings(double *out, int n);
/* device-side timings (HIP events) in the in-call-sampling and shard RANSAC
 * calls; off by default (host sampling time is always reported) */
int sfm_set_call_timing(int on);

/* ---------------------------------------------------------------------
 * Python `random` replay (host code, no GPU).
 * Replaces the n_max calls of random.sample(range(n), k) made by
 * GetInliersRANSAC.py:55 on the *global* MT19937 instance.  `mt_state`
 * is random.getstate()[1] (624 words + position) and is advanced in place
 * exactly as CPython 3.10 would (random.py:_randbelow_with_getrandbits and
 * sample()'s pool / set branches), so random.setstate() afterwards leaves
 * the global stream where the reference leaves it.  out: H x k int32.
 * ------------------------------------------------------------------- */
int sfm_pyrandom_sample_table(uint32_t *mt_state /* 625 in/out */, int64_t n, int32_t k,
                              int64_t H, int32_t *out);

/* ---------------------------------------------------------------------
 * EstimateFundamentalMatrix (EstimateFundamentalMatrix.py:3-83)
 * ------------------------------------------------------------------- */
/* H independent 8-point estimates: x1s, x2s are H x 8 x 2; F is H x 9. */
int sfm_f8_batch(const double *x1s, const double *x2s, int64_t H, double *F, int device);
/* one estimate from N >= 8 correspondences (least-squares null vector). */
int sfm_f8_general(const double *x1, const double *x2, int64_t N, double *F, int device);

/* ---------------------------------------------------------------------
 * GetInliersRANSAC (GetInliersRANSAC.py:5-106)
 * x1, x2: N x 2; samples: H x 8 indices (host-drawn, see above).
 * counts_out (H, nullable): inliers per hypothesis.  *best_iter: first
 * hypothesis with the strictly largest positive count, or -1 if every
 * count is 0 (the reference's "F_best is None").  F_best (9) and
 * best_mask (N, 1 = inlier) are written only when *best_iter >= 0.
 * ------------------------------------------------------------------- */
int sfm_ransac_f8(const double *x1, const double *x2, int64_t N, const int32_t *samples, int64_t H,
                  double thr, int32_t *counts_out, int64_t *best_iter, double *F_best,
                  uint8_t *best_mask, int device);
/* The same call with the H x 8 samples drawn inside it from the CPython
 * random state st[625] (random.getstate()[1]: 624 MT19937 words + position;
 * advanced in place exactly as H calls of random.sample(range(N), 8) would
 * advance it).  The draw is replayed on the host in chunks and each chunk's
 * upload / fit / score is enqueued as soon as it is drawn, so the GPU works
 * while the host draws.  samples_out (H x 8, nullable) receives the table. */
int sfm_ransac_f8_pyrandom(const double *x1, const double *x2, int64_t N, uint32_t *st, int64_t H,
                           double thr, int32_t *counts_out, int64_t *best_iter, double *F_best,
                           uint8_t *best_mask, int32_t *samples_out, int device);
/* GetInliersRANSAC's whole call (GetInliersRANSAC.py:53-106) as the drop-in
 * needs it: sfm_ransac_f8_pyrandom with the winner's inlier positions
 * (ascending) in split[0, *n_inliers) and the outliers' positions in
 * split[*n_inliers, N) (split: N entries) in place of the mask;
 * *n_inliers = 0 when *best_iter is -1. */
int sfm_ransac_f8_dropin(const double *x1, const double *x2, int64_t N, uint32_t *st, int64_t H, double thr,
                         int64_t *best_iter, double *F_best, int64_t *split, int64_t *n_inliers, int device);

/* ---------------------------------------------------------------------
 * Homography (GetHomographyInliers.py)
 * sfm_h4_batch: find_homography (:4-85) on H independent 4-point samples
 *   (x1s, x2s: H x 4 x 2) -> Hout (H x 9), each normalised by H[2,2].
 * sfm_homography_general: find_homography on N >= 4 points -> Hout (9).
 * sfm_ransac_h4: get_homography_inliers' loop (:124-157) over a host-drawn
 *   H x 4 sample table: per hypothesis the transfer error
 *   |H x1 / (t2 + 1e-8) - x2| < thr is counted; the winner is the first
 *   hypothesis with the strictly largest positive count (-1 if none);
 *   H_best (9) and best_mask (N) are written when *best_iter >= 0.
 * ------------------------------------------------------------------- */
int sfm_h4_batch(const double *x1s, const double *x2s, int64_t H, double *Hout, int device);
int sfm_homography_general(const double *x1, const double *x2, int64_t N, double *Hout, int device);
int sfm_ransac_h4(const double *x1, const double *x2, int64_t N, const int32_t *samples, int64_t H,
                  double thr, int32_t *counts_out, int64_t *best_iter, double *H_best,
                  uint8_t *best_mask, int device);
/* sfm_ransac_h4 with in-call sampling (H x 4), as sfm_ransac_f8_pyrandom. */
int sfm_ransac_h4_pyrandom(const double *x1, const double *x2, int64_t N, uint32_t *st, int64_t H,
                           double thr, int32_t *counts_out, int64_t *best_iter, double *H_best,
                           uint8_t *best_mask, int32_t *samples_out, int device);

/* ---------------------------------------------------------------------
 * PnP (LinearPnP.py, PnPRANSAC.py, NonlinearPnP.py); K is 3x3 row-major.
 * sfm_linear_pnp: LinearPnP on N >= 4 points (X: N x 3, x: N x 2) ->
 *   C (3), R (9); *branch (nullable) = 1 where R's final orthogonalisation
 *   is the LAPACK-noise-defined case (det(R) < 0).
 * sfm_pnp_ransac: PnPRANSAC's loop (:48-80) over a host-drawn H x 4 sample
 *   table: LinearPnP per hypothesis, reprojection error < thr counted;
 *   *best_iter = first strict maximum (-1 if every count is 0) and
 *   *best_count its count -- the caller applies the reference's fallback
 *   (:82-87, LinearPnP on all points when best_count < 4).
 * sfm_nonlinear_pnp: NonlinearPnP (:47-123), scipy 'lm' semantics with
 *   max_nfev on the 2N-residual loss (:5-44); info: MINPACK info, 0 for the
 *   N < 4 early return, -1 where the reference's except keeps (C0, R0); a
 *   non-negative info carries the CholeskyQR flags in bits 8-9 (1: the
 *   Jacobian's Gram factor needed a shift and a third pass ran; 2: a later
 *   Gram factor failed) -- info & 0xff is MINPACK's code.
 * ------------------------------------------------------------------- */
int sfm_linear_pnp(const double *X, const double *x, int64_t N, const double *K, double *C_out,
                   double *R_out, int32_t *branch, int device);
int sfm_pnp_ransac(const double *X, const double *x, int64_t N, const double *K, const int32_t *samples,
                   int64_t H, double thr, int32_t *counts_out, int32_t *branch_out, int64_t *best_iter,
                   int64_t *best_count, double *C_best, double *R_best, int device);
int sfm_nonlinear_pnp(const double *X, const double *x, int64_t N, const double *K, const double *C0,
                      const double *R0, int32_t max_nfev, double *C_out, double *R_out, int32_t *info,
                      int device);

/* ---------------------------------------------------------------------
 * Matching files (Utils.py:8-64 get_data) -> COO observation store.
 * sfm_matching_parse: reads data_path/matching1..(no_of_images-1).txt with
 *   get_data's semantics (header skipped; primary x, y as floats; match
 *   coordinates int()-truncated; last write per image wins) using
 *   n_threads host threads (0 = up to 16); returns an opaque store with
 *   n_features rows and n_obs observations (feature-major, image ascending).
 * sfm_matching_read: copies the COO arrays (feature, image 0-based, x, y).
 * ------------------------------------------------------------------- */
int sfm_matching_parse(const char *data_path, int32_t no_of_images, int32_t n_threads, void **handle,
                       int64_t *n_features, int64_t *n_obs);
int sfm_matching_read(void *handle, int32_t *feature, int32_t *image, double *x, double *y);
int sfm_matching_free(void *handle);

/* ---------------------------------------------------------------------
 * Dense visibility -> COO observations (BundleAdjustment.py:164-169, the
 * drop-in's np.where over filtered_feature_flags[valid_point_indices]
 * [:, :n_cameras] == 1 and the feature_x / feature_y gathers at the hits).
 * sfm_dense_obs_scan: rows[i] (i < n_rows) are the valid feature rows, each
 *   in [0, n_matrix_rows) (SFM_ERR_ARG otherwise: the matrices' row count,
 *   where the reference's indexing raises IndexError); a row r of the flag matrix starts at flags + r * flag_row_bytes (dtype
 *   0 f64, 1 f32, 2 i64, 3 i32, 4 u8/bool; "== 1" in that dtype), of the
 *   coordinate matrices at fx / fy + r * xy_row_bytes (f64); n_threads
 *   row jobs on the library's host threads (0 = its default).  Returns a
 *   store of n_obs observations in np.where's order (point-major, camera
 *   ascending), kept by the library for the next scan once freed.
 * sfm_dense_obs_read: copies (camera, point i, (x, y)).
 * sfm_ba_lm_dense (below) solves from the store without these copies.
 * ------------------------------------------------------------------- */
int sfm_dense_obs_scan(const void *flags, int32_t dtype, int64_t flag_row_bytes, int64_t n_matrix_rows,
                       const int64_t *rows, int64_t n_rows, int32_t n_cams, const double *fx, const double *fy,
                       int64_t xy_row_bytes, int32_t n_threads, void **handle, int64_t *n_obs);
int sfm_dense_obs_read(void *handle, int32_t *cam, int32_t *pt, double *obs);
int sfm_dense_obs_free(void *handle);
/* perform_bundle_adjustment's x0 points (BundleAdjustment.py:196-197):
 * dst[i] = src[rows[i]] for 3-double rows (rows NULL: src[i]), on the host
 * thread pool; SFM_ERR_ARG for a row outside [0, src_rows). */
int sfm_gather_rows3(const double *src, int64_t src_rows, const int64_t *rows, int64_t n, double *dst);
/* The camera parameter conversions around the solve (BundleAdjustment.py:
 * 183-193 and 220-228), scipy's Rotation with its bits (csrc/rotations.cpp):
 * sfm_matrix_to_rotvec = from_matrix(R).as_rotvec() for n row-major 3 x 3
 * matrices, returning how many are not orthogonal to within 1e-13 (scipy
 * orthogonalises those first: nothing is written for them, the caller
 * converts the batch with scipy), -1 for a null pointer / negative n;
 * sfm_rotvec_to_matrix = from_rotvec(w).as_matrix(). */
int64_t sfm_matrix_to_rotvec(const double *R, int64_t n, double *w);
int sfm_rotvec_to_matrix(const double *w, int64_t n, double *R);

/* ---------------------------------------------------------------------
 * LinearTriangulation (LinearTriangulation.py:3-92)
 * P1, P2: 3 x 4 projection matrices K[R | -RC]; x1, x2: N x 2; X: N x 3.
 * ------------------------------------------------------------------- */
int sfm_triangulate_dlt(const double *P1, const double *P2, const double *x1, const double *x2,
                        int64_t N, double *X, int device);

/* ---------------------------------------------------------------------
 * Two-view initialisation (ExtractCameraPose.py's candidates through
 * LinearTriangulation.py and DisambiguateCameraPose.py:45-91).
 * M pose candidates (1 <= M <= 8, else SFM_ERR_ARG) for camera 2: P2s
 * (M x 3 x 4 projection matrices K[R | -RC], formed by the caller as for
 * sfm_triangulate_dlt), Rs (M x 3 x 3), Cs (M x 3); camera 1: P1, R1, C1.
 * A point counts for candidate m when it lies in front of both cameras:
 * R1[2].(X - C1) > 0 and Rs[m][2].(X - Cs[m]) > 0.  *best: the first
 * candidate with the strictly largest count (DisambiguateCameraPose.py:77).
 * N == 0: every count 0, *best = 0.
 * sfm_two_view_select: one launch triangulates x1, x2 (N x 2, uploaded once)
 *   under every candidate and counts; X_best (N x 3) receives the winner's
 *   points, X_all (M x N x 3, nullable) every candidate's.
 * sfm_cheirality_count: the count alone on points already triangulated,
 *   Xset (M x N x 3).
 * ------------------------------------------------------------------- */
int sfm_two_view_select(const double *P1, const double *P2s, const double *R1, const double *C1,
                        const double *Rs, const double *Cs, int32_t M, const double *x1, const double *x2,
                        int64_t N, int64_t *counts, int32_t *best, double *X_best, double *X_all, int device);
int sfm_cheirality_count(const double *R1, const double *C1, const double *Rs, const double *Cs, int32_t M,
                         const double *Xset, int64_t N, int64_t *counts, int32_t *best, int device);

/* ---------------------------------------------------------------------
 * NonLinearTriangulation (NonLinearTriangulation.py:53-121): per point,
 * scipy least_squares(method='lm', max_nfev) of the 4-residual Loss
 * (:5-50) from X0[i]; MINPACK lmdif semantics (diag = ones, factor 100,
 * forward differences, ftol = xtol = gtol = 1e-8).  Rows where the
 * reference's try/except keeps X0 (x0 with a NaN, non-finite residuals at
 * x0) are copied through.  info (N, nullable): MINPACK info 1..8, or -1
 * for a copied-through row.
 * ------------------------------------------------------------------- */
int sfm_triangulate_nonlinear(const double *P1, const double *P2, const double *x1, const double *x2,
                              const double *X0, int64_t N, int32_t max_nfev, double *X, int32_t *info,
                              int device);

/* ---------------------------------------------------------------------
 * Multi-view track triangulation: one point per track from ALL of its views
 * in one launch (the reference's registration loop, Wrapper_dev.py:262-291,
 * triangulates image pairs one at a time and keeps the last pair's point).
 * P: n_cams x 3 x 4 projection matrices K[R | -RC].  Tracks are CSR rows:
 * track t owns observations [track_start[t], track_start[t+1]) of obs_cam
 * (camera index) and obs_xy (n_obs x 2), cameras ascending within a track;
 * track_start has T + 1 entries, starts at 0, never decreases and ends at
 * n_obs, and every camera index lies in [0, n_cams) -- else SFM_ERR_ARG,
 * checked on the host before anything is launched.  X0 (T x 3) is nullable
 * except in SFM_TRACKS_REFINE mode.
 * mode: SFM_TRACKS_LINEAR the N-view DLT (LinearTriangulation.py:54-90's
 *   two rows per view, least singular vector, divided where |h3| > 1e-8);
 *   SFM_TRACKS_REFINE Levenberg-Marquardt from X0 on the 2n residuals
 *   u - h0/h2, v - h1/h2 (NonLinearTriangulation.py:5-50's loss over all
 *   views; a view with |h2| < 1e-8 contributes none), ftol = xtol = gtol =
 *   1e-8, at most max_nfev cost evaluations, only steps that lower the cost
 *   accepted; SFM_TRACKS_BOTH the first, then the second from its result.
 * A two-view track returns sfm_triangulate_dlt's and
 * sfm_triangulate_nonlinear's bits.
 * Outputs per track: X (T x 3); cost (T), the sum of squared residuals at X;
 * front (T), 1 where X lies in front of every camera of the track (h2 > 0);
 * info (T): >= 1 the refinement's stop code (1 ftol, 2 xtol, 3 both, 4 gtol,
 * 5 max_nfev; MINPACK's info for a two-view track), 0 in SFM_TRACKS_LINEAR
 * mode, -1 where the refinement's start has a NaN or residuals that are not
 * finite (X is the start), -2 for a track of fewer than two views (X is
 * X0's row where X0 is given and zeros otherwise, cost 0, front 0).
 * The projections are staged in LDS up to SFM_TRACKS_LDS_CAMS cameras and
 * read from global memory above; the results do not depend on which.
 * T == 0 returns 0 without touching a device.
 * ------------------------------------------------------------------- */
#define SFM_TRACKS_LDS_CAMS 64
enum { SFM_TRACKS_LINEAR = 0, SFM_TRACKS_REFINE = 1, SFM_TRACKS_BOTH = 2 };
int sfm_triangulate_tracks(const double *P, int32_t n_cams, const int64_t *track_start, int64_t T,
                           const int32_t *obs_cam, const double *obs_xy, int64_t n_obs, const double *X0,
                           int32_t mode, int32_t max_nfev, double *X, double *cost, uint8_t *front,
                           int32_t *info, int device);

/* ---------------------------------------------------------------------
 * Robust multi-view track triangulation: sfm_triangulate_tracks trusts every
 * observation; this finds, per track, the observations that agree on one
 * point, fits the point to those alone and reports which they are.  The
 * reference has no counterpart.  P, the CSR tracks and their checks are
 * sfm_triangulate_tracks's; centres (n_cams x 3, nullable) are the camera
 * centres, used for `angle` only.
 * Hypotheses of a track of n >= 2 views are view pairs (i, j), i < j,
 * positions inside the track, enumerated by decreasing index gap g = n-1 ..
 * 1 and for each gap i = 0 .. n-1-g, the first max_pairs of them.  A pair's
 * point is sfm_triangulate_dlt's for its two observations; one that is not
 * finite counts 0.  An observation (u, v) is an inlier of a point with
 * projection h where h2 > 0, not |h2| < 1e-8 and (u - h0/h2)^2 +
 * (v - h1/h2)^2 < threshold^2.  The winner has the most inliers, then the
 * smallest sum of its inliers' squared errors (added in observation order),
 * then the earliest place in the enumeration.
 * The winner's inliers are refitted as sfm_triangulate_tracks
 * (SFM_TRACKS_BOTH) fits a track of those observations alone, bit for bit:
 * three or more by the N-view DLT and Levenberg-Marquardt, exactly two by the
 * two-view bodies.  The mask is then recomputed once against the refitted X.
 * Outputs per track: X (T x 3); cost (T), the sum of the final inliers'
 * squared errors; n_inliers (T); best_pair (T), the winner's place in the
 * enumeration or -1; best_count (T), its inlier count; info (T): >= 1 the
 * refinement's stop code and -1 as in sfm_triangulate_tracks, -2 fewer than
 * two views (X zeros, nothing an inlier), -3 no hypothesis with min_inliers
 * inliers (X is the best hypothesis's unrefined point; the mask, n_inliers
 * and cost are that hypothesis's own); angle (T, nullable, and null where
 * centres is null), the largest angle in radians between the rays X - C_i,
 * X - C_j over pairs of final inliers (0 with fewer than two).  Nothing is
 * gated on angle.  Per observation: inlier (n_obs), 1 or 0.
 * threshold is in pixels, finite and > 0; max_pairs >= 1; min_inliers >= 2;
 * max_nfev > 0.  lanes_per_track: the lanes of a wave that share one track's
 * hypotheses, a power of two up to 64, or 0 to choose from the tracks'
 * lengths and number; the results do not depend on it, nor on whether the
 * projections are staged in LDS (n_cams <= SFM_TRACKS_LDS_CAMS).
 * Every argument is checked on the host before anything is launched; T == 0
 * returns 0 without touching a device.
 * ------------------------------------------------------------------- */
int sfm_triangulate_tracks_robust(const double *P, int32_t n_cams, const double *centres,
                                  const int64_t *track_start, int64_t T, const int32_t *obs_cam,
                                  const double *obs_xy, int64_t n_obs, double threshold, int32_t max_pairs,
                                  int32_t min_inliers, int32_t max_nfev, int32_t lanes_per_track, double *X,
                                  double *cost, int32_t *n_inliers, uint8_t *inlier, int32_t *best_pair,
                                  int32_t *best_count, int32_t *info, double *angle, int device);

/* ---------------------------------------------------------------------
 * Batched view registration: 6-point PnP RANSAC and a pose refit for every
 * candidate view in one call (the reference registers one image per call from
 * 4-point samples, Wrapper_dev.py:232-249; differs on purpose).
 * K 3 x 3; X (n_pts x 3) the points.  The V views are CSR rows: view v owns
 * correspondences [view_start[v], view_start[v+1]) of pt_idx (index into X) and
 * xy (n_corr x 2); view_start has V + 1 entries, starts at 0, never decreases
 * and ends at n_corr, every pt_idx lies in [0, n_pts).  samples (V x H x 6):
 * each entry a position inside its view, in [0, n_v), the six of a hypothesis
 * distinct; ignored for views of n_v < 6.  A violation is SFM_ERR_ARG, found on
 * the host before anything is launched.
 * Hypothesis: the 12 x 12 DLT system of the six sampled correspondences, its
 * right singular vector of the smallest singular value (one-sided Jacobi),
 * [M | t] with the sign that makes det M > 0, split as M = L R (L lower
 * triangular, positive diagonal; det R = 1), scale = mean(diag L), C = -R^T t /
 * scale.  The hypothesis is scored under its own projection P = K [M | t] /
 * scale, the 11-parameter fit of its six points (`models`); (C, R) is the pose
 * the refit starts from.  One whose model is not finite scores 0.  An observation (u, v) is an inlier of P where, with
 * h = P [X; 1], h2 > 0, not |h2| < 1e-8 and (u - h0/h2)^2 + (v - h1/h2)^2 <
 * threshold^2 (the fp64 expression decides).  The winner has the most inliers,
 * then the earliest place in the table.
 * Refit: Levenberg-Marquardt on six pose parameters (rotation increment
 * multiplied from the left, C additive) over the current inliers, lambda 1e-3,
 * / 10 on an accepted and x 10 on a rejected step, only steps that lower the
 * cost accepted, MINPACK's stop tests at 1e-8 and at most max_nfev cost
 * evaluations; every correspondence of the view is then scored against the
 * refitted pose, and (count, then smaller cost) replaces the current state only
 * if it is not worse; up to refit_rounds rounds, ending early when the mask does
 * not change.  So n_inliers >= best_count.
 * Outputs per view: C (V x 3), R (V x 9), cost (sum of the final inliers'
 * squared errors), n_inliers, best_hyp (-1 without one), best_count, info:
 * 1..5 the last refit's stop code (1 ftol, 2 xtol, 3 both, 4 gtol, 5 max_nfev),
 * 0 refit_rounds = 0, -1 n_v < 6 (C = 0, R = I, nothing an inlier; nothing of
 * the view is read on or from the device), -2 no finite hypothesis (the same
 * outputs), -3 best_count < min_inliers (the winning hypothesis's pose, mask,
 * count and cost, no refit), -4 the refit's start had no finite cost (as -3).
 * Per correspondence: inlier (n_corr), 1 or 0.  Nullable: counts (V x H) the
 * inliers per hypothesis, models (V x H x 12) the hypothesis projections; both
 * zero for a view of n_v < 6.
 * threshold is in pixels, finite and > 0; H >= 1; min_inliers >= 6;
 * refit_rounds >= 0; max_nfev > 0.  No sum depends on the batch: a view's
 * outputs are the same bits alone, in any batch and at any place in it.
 * Two launches and one synchronisation whatever V is; V == 0, or no view of six
 * correspondences, returns without touching a device.  sfm_last_timings: upload,
 * both kernels, download, the fit-and-score kernel alone.
 * ------------------------------------------------------------------- */
int sfm_register_views(const double *K, const double *X, int64_t n_pts, const int64_t *view_start, int64_t V,
                       const int32_t *pt_idx, const double *xy, int64_t n_corr, const int32_t *samples,
                       int64_t H, double threshold, int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev,
                       double *C, double *R, double *cost, int32_t *n_inliers, int32_t *best_hyp,
                       int32_t *best_count, int32_t *info, uint8_t *inlier, int32_t *counts, double *models,
                       int device);

/* ---------------------------------------------------------------------
 * Calibrated batched view registration: sfm_register_views with the minimal
 * solver of a calibrated camera, 3-point samples and up to four poses per
 * hypothesis (the reference has no counterpart).  It registers views whose
 * points lie on one plane, where the 12 x 12 DLT system of sfm_register_views
 * has a four-dimensional null space.
 * K, X, view_start, pt_idx, xy: as sfm_register_views, under the same rules.
 * samples (V x H x 3): each entry a position inside its view, in [0, n_v), the
 * three of a hypothesis distinct; ignored for views of n_v < 4.  1 <= H <=
 * 2^20; threshold in pixels, finite and > 0; min_inliers >= 4 (a view of three
 * correspondences fits every solution exactly and decides nothing);
 * refit_rounds >= 0; max_nfev > 0.  A violation is SFM_ERR_ARG, found on the
 * host before a device is looked for; no output is touched.
 * Hypothesis: bearings b_i = K^-1 [x_i; 1], normalised.  Every pose (R, C) with
 * det R = +1 is a solution for which R (X_i - C) is a positive multiple of b_i
 * for the three sampled correspondences and which is finite; there are up to
 * four, n_sol (V x H) counts them.  Their set is specified, their order is not.
 * Method (csrc/p3p.hpp): with a_ij = |X_i - X_j|^2 / extent^2 (extent the
 * largest of the three distances) and c_ij = b_i . b_j the depths d_i satisfy
 * d_i^2 + d_j^2 - 2 c_ij d_i d_j = a_ij; the real roots of the cubic det(D1 + g
 * D2) = 0 of the two homogeneous combinations D1, D2 of these quadrics are
 * found (one by Newton's method from a bound it approaches monotonically, the
 * other two from the remaining quadratic, real where its discriminant is >= 0)
 * and polished by two Newton steps; the root whose
 * degenerate quadric is most clearly a pair of real planes is taken, and each
 * plane cuts the other quadric of the pencil in a homogeneous quadratic.  A
 * root of a quadratic counts as real where its discriminant is >= 0 in fp64.
 * Every candidate is polished by five Gauss-Newton steps on the three distance
 * constraints and kept where its depths are finite and positive and every
 * constraint holds to 1e-10 (of a_ij <= 1) afterwards, so that a root that is
 * real by rounding alone is dropped.  R maps the orthonormal frame of the
 * triangle X to that of the triangle d_i b_i; C = mean X - R^T mean(d b).
 * A sample has no solutions (n_sol = 0, no error) where two of its points lie
 * within 1e-12 of the sample's extent of each other or its three points are
 * collinear in space (|(X_2 - X_1) x (X_3 - X_1)| <= 1e-10 extent^2).
 * Score: every solution under P = K [R | -R C], the pose itself (`models`),
 * with sfm_register_views' inlier rule: with h = P [X; 1], h2 > 0, not |h2| <
 * 1e-8 and (u - h0/h2)^2 + (v - h1/h2)^2 < threshold^2 (the fp64 expression
 * decides).  The winner over all (hypothesis, solution) pairs has the most
 * inliers, then the smaller sum of its inliers' squared errors, then the
 * earlier hypothesis, then the earlier solution.  The cost is formed only for
 * the solutions that tie on the best count, one pass over the view's
 * correspondences each in the view's one workgroup: the winner's selection
 * costs (1 + ties) passes, up to 4 H of them where every solution of every
 * hypothesis has the best count (a noise-free view).
 * Refit: sfm_register_views' own, started from the winning solution's pose: LM
 * on six pose parameters over the current inliers under the same control and
 * stop codes, the re-score of the whole view, the not-worse rule, up to
 * refit_rounds rounds.  So n_inliers >= best_count.
 * Outputs per view: C, R, cost, n_inliers, best_hyp (the winner's hypothesis,
 * -1 without one), best_count, info as sfm_register_views with -1 n_v < 4 (C =
 * 0, R = I, nothing an inlier; nothing of the view is read on or from the
 * device), -2 no solution in any hypothesis (the same outputs), -3 best_count <
 * min_inliers (the winning solution's pose, mask, count and cost, no refit),
 * -4 the refit's start had no finite cost (as -3).  Per correspondence: inlier
 * (n_corr), 1 or 0.  Nullable: n_sol (V x H), counts (V x H x 4) the inliers
 * per solution, models (V x H x 4 x 12) the projections; counts and models are
 * zero in the slots past n_sol, and all three are zero for a view of n_v < 4.
 * No sum depends on the batch and there are no float atomics: a view's outputs
 * are the same bits alone, in any batch and at any place in it, and a
 * hypothesis's n_sol, counts and models do not depend on H.  Two launches and
 * one synchronisation whatever V is; V == 0, or no view of four
 * correspondences, returns without touching a device.  sfm_last_timings:
 * upload, both kernels, download, the fit-and-score kernel alone.
 * ------------------------------------------------------------------- */
int sfm_register_views_p3p(const double *K, const double *X, int64_t n_pts, const int64_t *view_start, int64_t V,
                           const int32_t *pt_idx, const double *xy, int64_t n_corr, const int32_t *samples,
                           int64_t H, double threshold, int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev,
                           double *C, double *R, double *cost, int32_t *n_inliers, int32_t *best_hyp,
                           int32_t *best_count, int32_t *info, uint8_t *inlier, int32_t *n_sol, int32_t *counts,
                           double *models, int device);

/* ---------------------------------------------------------------------
 * Batched pair verification: 8-point F-RANSAC and a least-squares refit for
 * every image pair in one call, under one convention, x2^T F x1 = 0 (the
 * reference verifies one pair per call, Wrapper_dev.py:69-123, with a design
 * row for x1^T F x2 = 0 under a score for x2^T F x1 = 0, which the drop-ins
 * keep bit for bit; differs on purpose).
 * The P pairs are CSR rows: pair p owns correspondences [pair_start[p],
 * pair_start[p+1]) of x1 and x2 (n_corr x 2 each: pixel coordinates in the
 * pair's first and second image); pair_start has P + 1 entries, starts at 0,
 * never decreases and ends at n_corr.  samples (P x H x 8): each entry a
 * position inside its pair, in [0, n_p), the eight of a hypothesis distinct;
 * ignored for pairs of n_p < 8.  A violation is SFM_ERR_ARG, found on the host
 * before anything is launched.
 * Hypothesis: Hartley normalisation of the eight points on each side (centroid
 * to the origin, mean distance sqrt 2), the design row [c a, c b, c, d a, d b,
 * d, a, b, 1] with (a, b) the normalised first point and (c, d) the second,
 * the null vector of the 8 x 9 system as F^ (row-major), projected to rank 2,
 * F = T2^T F^ T1, scaled to unit Frobenius norm with the sign that makes the
 * entry of largest magnitude (the first such in row-major order) positive; no
 * division by F[2,2].  One whose model is not finite scores 0.
 * A correspondence is an inlier of F where, with e = x2^T F x1 and den =
 * (F x1)_0^2 + (F x1)_1^2 + (F^T x2)_0^2 + (F^T x2)_1^2, den > 0 and e e <
 * threshold^2 den: the squared Sampson distance against the squared threshold,
 * without a division or a square root (the fp64 expression decides).  The
 * winner has the most inliers, then the earliest place in the table.
 * Refit: the normalised least-squares fit over the current inliers (the same
 * design, N x 9, Hartley statistics of the inliers on each side; Givens QR to
 * a 9 x 9 triangular factor, its right singular vector of the least singular
 * value by one-sided Jacobi), then rank 2, denormalisation, scale and sign as
 * for a hypothesis; every correspondence of the pair is scored against it, and
 * (count, then smaller cost) replaces the current state only if it is not
 * worse; up to refit_rounds rounds, ending early when the mask does not change,
 * when the new state is worse or when fewer than 8 inliers remain.  So
 * n_inliers >= best_count.
 * Outputs per pair: F (P x 9, row-major), cost (the sum of the final inliers'
 * squared Sampson distances e e / den), n_inliers, best_hyp (-1 without one),
 * best_count, info: 1 the refit ended on an unchanged mask, 2 it ended on a
 * worse state or refit_rounds ran out, 0 refit_rounds = 0, -1 n_p < 8 (F = 0,
 * nothing an inlier; nothing of the pair is read on or from the device), -2 no
 * finite hypothesis (the same outputs), -3 best_count < min_inliers (the
 * winning hypothesis's F, mask, count and cost, no refit).
 * Per correspondence: inlier (n_corr), 1 or 0.  Nullable: counts (P x H) the
 * inliers per hypothesis, models (P x H x 9) the hypotheses; both zero for a
 * pair of n_p < 8.
 * threshold is in pixels, finite and > 0; H >= 1; min_inliers >= 8;
 * refit_rounds >= 0.  No sum depends on the batch: a pair's outputs are the
 * same bits alone, in any batch and at any place in it.  Two launches and one
 * synchronisation whatever P is; P == 0, or no pair of eight correspondences,
 * returns without touching a device.  sfm_last_timings: upload, both kernels,
 * download, the fit-and-score kernel alone.
 * ------------------------------------------------------------------- */
int sfm_verify_pairs(const int64_t *pair_start, int64_t P, const double *x1, const double *x2, int64_t n_corr,
                     const int32_t *samples, int64_t H, double threshold, int32_t min_inliers,
                     int32_t refit_rounds, double *F, double *cost, int32_t *n_inliers, int32_t *best_hyp,
                     int32_t *best_count, int32_t *info, uint8_t *inlier, int32_t *counts, double *models,
                     int device);

/* ---------------------------------------------------------------------
 * Batched calibrated pair verification: 5-point essential-matrix RANSAC and a
 * five-parameter refit for every image pair in one call, under
 * sfm_verify_pairs' convention (x2^T F x1 = 0, unit-norm models, the Sampson
 * distance in pixels).  The reference has no counterpart.  Unlike the 8-point F
 * the model exists for a pair that sees one plane.  Pure rotation (t = 0, E
 * undefined) is out of scope.
 * K 3 x 3, finite, with a non-zero determinant; K^-1 is formed once on the host
 * by the adjugate.  The P pairs are CSR rows exactly as for sfm_verify_pairs:
 * pair_start (P + 1), x1 and x2 (n_corr x 2).  samples (P x H x 5): each entry a
 * position inside its pair, in [0, n_p), the five of a hypothesis distinct;
 * ignored for pairs of n_p < 5.  threshold is in pixels, finite and > 0; 1 <= H
 * <= 2^20; min_inliers >= 5; refit_rounds >= 0; max_nfev > 0.  A violation is
 * SFM_ERR_ARG, found on the host before anything is launched, with no output
 * touched.
 * Hypothesis: with x^ = K^-1 [x; 1] (dehomogenised), the 5 x 9 system of design
 * rows [c a, c b, c, d a, d b, d, a, b, 1], (a, b) = x^1 and (c, d) = x^2, so that
 * x^2^T E x^1 = 0 for E row-major; an orthonormal basis X, Y, Z, W of its
 * four-dimensional null space (Householder); every E = x X + y Y + z Z + W with
 * det E = 0 and 2 E E^T E - tr(E E^T) E = 0.  These ten cubics over the 20
 * monomials are reduced by Gauss-Jordan with partial pivoting on the ten
 * columns that hold x or y to a power of two or more, which leaves B(z) [x, y,
 * 1]^T = 0 with a 3 x 3 polynomial matrix; the roots of det B, of degree 10,
 * are found by Aberth iteration from fixed starting points (at most 64 sweeps),
 * a root counts as real where |Im z| <= 1e-8 max(1, |Re z|) and is polished by
 * three Newton steps; x and y follow from the null vector of B(z).  Each
 * solution is scaled to unit Frobenius norm with the sign that makes the entry
 * of largest magnitude (the first such in row-major order) positive; solutions
 * that are not finite are dropped.  There are up to ten per hypothesis: n_sol
 * counts them, and only their set is specified, not their order.
 * Score: F = K^-T E K^-1 brought to unit norm and sign in the same way, then
 * sfm_verify_pairs' inlier rule, e e < threshold^2 den with den > 0 (the fp64
 * expression decides).  The winner over all (hypothesis, solution) pairs has
 * the most inliers, then the smaller sum of the inliers' squared Sampson
 * distances, then the earlier hypothesis (then the earlier solution).
 * Refit: E = +-s [t]x R by one-sided Jacobi (R = U W V^T, negated where its
 * determinant is negative; t = u3), then Levenberg-Marquardt on five
 * parameters -- a rotation increment multiplied from the left, and t moved in
 * the tangent plane of the unit sphere spanned by b1 = t x e_k / |t x e_k| (k
 * the axis of the smallest |t_k|, the first of equals) and b2 = t x b1, then
 * renormalised -- over the current inliers' Sampson distances e / sqrt(den) in
 * pixels, controlled as sfm_register_views' refit: lambda 1e-3, / 10 on an
 * accepted and x 10 on a rejected step, only steps that lower the cost
 * accepted, MINPACK's stop tests at 1e-8 and at most max_nfev cost evaluations.
 * Every correspondence of the pair is then scored against the refitted E, and
 * (count, then smaller cost) replaces the current state only if it is not
 * worse; up to refit_rounds rounds, ending early when the mask does not
 * change.  So n_inliers >= best_count.
 * Outputs per pair: E (P x 9) and F (P x 9), row-major, both of unit norm, F =
 * K^-T E K^-1 up to scale (F goes straight into sfm_init_pairs); cost (the sum
 * of the final inliers' squared Sampson distances), n_inliers, best_hyp (-1
 * without one), best_count, info: 1..5 the last refit's stop code (1 ftol, 2
 * xtol, 3 both, 4 gtol, 5 max_nfev), 0 refit_rounds = 0, -1 n_p < 5 (E = F = 0,
 * nothing an inlier; nothing of the pair is read on or from the device), -2 no
 * finite solution in any hypothesis (the same outputs), -3 best_count <
 * min_inliers (the winning solution's E, F, mask, count and cost, no refit), -4
 * the refit's start had no finite cost or E no factorisation (as -3).
 * Per correspondence: inlier (n_corr), 1 or 0.  Nullable: n_sol (P x H), counts
 * (P x H x 10) the inliers per solution, models (P x H x 10 x 9) the solutions
 * E; the slots past n_sol are zero, and all three are zero for a pair of n_p <
 * 5.
 * No sum depends on the batch and there are no float atomics: a pair's outputs
 * are the same bits alone, in any batch and at any place in it, and a
 * hypothesis's n_sol, counts and models do not depend on H.  Two launches and
 * one synchronisation whatever P is; P == 0, or no pair of five
 * correspondences, returns without touching a device.  sfm_last_timings:
 * upload, both kernels, download, the fit-and-score kernel alone.
 * ------------------------------------------------------------------- */
int sfm_essential_pairs(const double *K, const int64_t *pair_start, int64_t P, const double *x1,
                        const double *x2, int64_t n_corr, const int32_t *samples, int64_t H, double threshold,
                        int32_t min_inliers, int32_t refit_rounds, int32_t max_nfev, double *E, double *F,
                        double *cost, int32_t *n_inliers, int32_t *best_hyp, int32_t *best_count, int32_t *info,
                        uint8_t *inlier, int32_t *n_sol, int32_t *counts, double *models, int device);

/* ---------------------------------------------------------------------
 * Batched initial-pair selection: for every verified pair in one call, the
 * relative pose from its F, the cheirality counts of the four candidates, the
 * winner's points with their parallax angles and the support of the best
 * 4-point homography -- what tells a wide-baseline pair from one without
 * baseline or of a plane (the pair of most inliers is usually the former's
 * opposite).  The reference starts from its first two images and has no
 * counterpart; sfm_two_view_select serves one pair from host-built candidates.
 * K 3 x 3.  The P pairs are CSR rows as for sfm_verify_pairs: pair_start (P +
 * 1), x1 and x2 (n_corr x 2); every row given is used, so the caller passes the
 * verified inliers only.  F (P x 9, row-major) under x2^T F x1 = 0, as
 * sfm_verify_pairs returns it.  hsamples (P x Hh x 4): each entry a position
 * inside its pair, in [0, n_p), the four of a hypothesis distinct; ignored for
 * pairs of n_p < 4; null exactly when Hh = 0.  h_threshold and max_reproj are
 * in pixels, finite and > 0; 0 <= Hh <= 2^20.  A violation is SFM_ERR_ARG,
 * found on the host before anything is launched.
 * Per pair, on the device in fp64:
 * Candidates: E = K^T F K = U diag(s) V^T by one-sided Jacobi; with W = [[0, -1,
 * 0], [1, 0, 0], [0, 0, 1]], R_a = U W V^T and R_b = U W^T V^T, each negated
 * where its determinant is negative; t = u3, the left singular vector of the
 * least singular value; the candidates are (R_a, t), (R_a, -t), (R_b, t), (R_b,
 * -t).  Camera 1 is K [I | 0], camera 2 K [R | t] with centre C = -R^T t, |C| =
 * 1.  Which place a candidate takes among the four follows the signs the
 * decomposition happens to return: only the set is specified.
 * Cheirality: every correspondence is triangulated under every candidate as
 * sfm_triangulate_dlt does and counts for it under sfm_two_view_select's rule
 * (in front of both cameras); counts (P x 4); best: the first candidate with
 * the strictly largest count.
 * Under the winner, per correspondence: X (n_corr x 3); good (n_corr), 1 where X
 * is finite, lies in front of both cameras and its squared reprojection error
 * is < max_reproj^2 in each image; angle (n_corr) = atan2(|a x b|, a.b) in
 * radians with a = X and b = X - C, 0 where not good (and where the expression
 * is not a number).  Per pair: R (P x 9) and C (P x 3) of the winner; n_good;
 * median_angle, the lower median of the good angles -- the element of sorted
 * index (n_good - 1) / 2, one of the pair's own angle values bit for bit (an
 * exact selection, no histogram estimate), 0 with none.
 * Homography support (Hh > 0): a hypothesis is the normalised 4-point DLT under
 * x2 ~ H x1 -- Hartley normalisation of the four points on each side, the rows
 * [0, 0, 0, -a, -b, -1, d a, d b, d] and [a, b, 1, 0, 0, 0, -c a, -c b, -c] with
 * (a, b) the normalised first point and (c, d) the second, the null vector of
 * the 8 x 9 system, H = T2^-1 H^ T1, scaled to unit Frobenius norm with the sign
 * that makes the entry of largest magnitude (the first such in row-major order)
 * positive; no division by H[2,2] (not find_homography's convention; differs on
 * purpose).  A correspondence is an inlier where, with h = H [x1; 1], h2 is
 * finite, |h2| >= 1e-12 and (u2 - h0/h2)^2 + (v2 - h1/h2)^2 < h_threshold^2.
 * The winner has the most inliers, then the earliest place in the table.
 * h_count, h_best (-1 without one: Hh = 0, or no hypothesis with an inlier),
 * Hbest (P x 9, zeros without a winner).
 * info (P): 0 done; -1 n_p < 8 (nothing of the pair is read on or from the
 * device, the homography stage included: R = I, C = 0, counts 0, best 0, X 0,
 * nothing good, angles 0, h_count 0, h_best -1, Hbest 0); -2 F or E is not
 * finite or the second singular value of E is 0 (the outputs of -1, but the
 * homography stage runs).
 * Nullable: cands (P x 4 x 12: R row-major, then t), hcounts (P x Hh), hmodels
 * (P x Hh x 9); zero for pairs that are not processed (cands: info < 0, the
 * other two: info -1).
 * Counts are integers and every other value comes from the pair alone: a pair's
 * outputs are the same bits alone, in any batch and at any place in it.  Two
 * launches (one with Hh = 0) and one synchronisation whatever P is; P == 0, or
 * no pair of eight correspondences, returns without touching a device.
 * sfm_last_timings: upload, both kernels, download, the homography kernel alone.
 * ------------------------------------------------------------------- */
int sfm_init_pairs(const double *K, const int64_t *pair_start, int64_t P, const double *x1, const double *x2,
                   int64_t n_corr, const double *F, const int32_t *hsamples, int64_t Hh, double h_threshold,
                   double max_reproj, double *R, double *C, int64_t *counts, int32_t *best, int32_t *n_good,
                   double *median_angle, int32_t *h_count, int32_t *h_best, double *Hbest, int32_t *info, double *X,
                   uint8_t *good, double *angle, double *cands, int32_t *hcounts, double *hmodels, int device);

/* ---------------------------------------------------------------------
 * Global rotation averaging: the rotation of every camera from the relative
 * rotations of the pairs, in one call -- one spanning tree, consensus sweeps
 * that repair it, a weighted refit on the consensus set.  sfm_init_pairs gives
 * a relative pose for every verified pair and the incremental chain uses one of
 * them; this uses all of them, and its edge mask is the loop-consistency check
 * on pairs that passed RANSAC with a wrong geometry.  The reference has no
 * counterpart.
 * n_images = N >= 0 cameras; the n_edges = E >= 0 edges are pair_ij (E x 2
 * int32: i != j, both in [0, N); duplicate pairs and both orientations of a
 * pair are allowed, each is an edge of its own) with R_rel (E x 3 x 3 fp64,
 * row-major) under R_j ~ R_rel R_i for x_cam = R (X - C): sfm_init_pairs' R of
 * the pair (i, j), whose camera i is [I | 0].  R_rel must hold rotations:
 * finiteness is checked, orthogonality is not.  weight (E, finite and > 0) is
 * nullable: every weight 1.  threshold, the inlier angle in radians, finite, in
 * (0, pi); consensus_sweeps >= 0; max_sweeps >= 0; tol >= 0 radians; E <= 2^30.
 * A violation is SFM_ERR_ARG, found on the host before a device is looked for,
 * with nothing written.
 * Definitions, from which every output follows; fp64 with no contraction:
 *   products: (A B)[r][c] = (A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c];
 *     with A^T or B^T the same three terms in the same order, the transposed
 *     factor read through swapped indices;
 *   adjacency: node n's entries are the edges that contain n, by ascending edge
 *     index e.  For e = (i, j): the entry (e, j, fwd) in i's list predicts
 *     R_i = R_rel^T R_j, the entry (e, i, rev) in j's list predicts
 *     R_j = R_rel R_i; P_a is the prediction of a node's entry a = 0 .. d - 1
 *     from the neighbour's current rotation;
 *   trace test of a prediction P against a matrix Q (another prediction or a
 *     rotation): with both row-major as p[0..8], q[0..8],
 *     t = (..((p0 q0 + p1 q1) + p2 q2) + ..) + p8 q8 -- the nine products of
 *     tr(P Q^T) added left to right -- and the test is t >= tau with
 *     tau = 1 + 2 cos(threshold), two fp64 operations on the C library's cos:
 *     the angle between P and Q is at most threshold;
 *   priority(seed, e), 64-bit unsigned arithmetic modulo 2^64:
 *     z = seed + (e + 1) 0x9E3779B97F4A7C15;
 *     z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9;
 *     z = (z ^ (z >> 27)) 0x94D049BB133111EB;  priority = z ^ (z >> 31);
 *   components and roots (host, union-find): each connected component of the
 *     graph of all edges has one root, its node of highest degree, the lowest
 *     index on ties; a node without edges is its own root.
 * Stage 1, spanning tree (device, level-synchronous breadth-first search from
 * all roots at once, as many levels as the graph is deep): a root has level 0
 * and R = I.  A node not yet reached with an entry whose neighbour has level l
 * gets level l + 1 and the prediction of the one such entry of smallest
 * (priority(seed, e), e).
 * Stage 2, consensus_sweeps Jacobi sweeps (every node reads the rotations of
 * the sweep before): for a node that is not a root,
 * support_a = #{ b : P_a passes the trace test against P_b } (b = a included),
 * and R becomes P_a for the a of greatest support, the lowest a on ties.  d^2
 * tests per node and sweep: the hot path.  One workgroup per node, of 64
 * threads (one wave) up to degree 64, 128 up to 128 and 256 above; thread a
 * keeps P_a in registers, the P_b pass through LDS in tiles of the workgroup's
 * size as 72-byte records, and a node of more entries than threads walks the
 * (a, b) tiles, forming each tile's predictions again from global memory.
 * Stage 3, refit: Jacobi sweeps over the nodes that are not roots.  For the
 * entries, in their order, whose P passes the trace test against the node's R
 * (t its sum): M = P R^T, v = ((M21 - M12) / 2, (M02 - M20) / 2, (M10 - M01) / 2),
 * s = sqrt((v0 v0 + v1 v1) + v2 v2), theta = atan2(s, (t - 1) / 2),
 * log = v (theta / s) (v where s = 0); num += w_e log per component and
 * den += w_e, left to right from 0; omega = num / den, theta_w = its norm (as
 * s), and R <- exp(omega) R with exp(omega) = I + A [omega]x + B [omega]x^2,
 * A = sin(theta_w) / theta_w and B = 2 sin^2(theta_w / 2) / theta_w^2 (1 -
 * theta_w^2 / 6 and 1/2 - theta_w^2 / 24 below 1e-4).  A node without a
 * passing entry keeps its R and counts omega = 0.  The sweeps end after the
 * first one whose largest theta_w <= tol, where tol > 0, or after max_sweeps;
 * tol = 0 runs exactly max_sweeps.  The largest theta_w is an integer maximum
 * over the bits of the doubles, no float atomic; later launches test it on the
 * device and the host looks every 8 sweeps.  One launch per sweep, no
 * grid-wide barrier.  The log is ill-conditioned for an angle next to pi, so a
 * threshold that admits such entries is allowed but not useful.
 * Outputs, caller-allocated: R (N x 3 x 3); per edge (i, j), with P = R_rel R_i
 * and t its trace sum against R_j: edge_inlier (E, 1 where t >= tau) and
 * edge_angle (E) = atan2(s, (t - 1) / 2) in radians, s from M = P R_j^T as in
 * stage 3; n_inlier_edges (N): a node's inlier edges; group (N): the connected
 * component of the graph of inlier edges, labelled by its lowest node (host
 * union-find after the download); info (N): 1 the root of a component with an
 * edge, 0 another node with an inlier edge, -1 a node with none, the nodes
 * without any edge included; level (N): the node's level in stage 1; *sweeps:
 * the refit sweeps run.
 * Gauge: the root of every component of the input graph is I.  The rotations
 * inside one group are mutually consistent; a group that lost its inlier
 * connection to its root keeps whatever offset the tree gave it, so a caller
 * uses one group (the largest).
 * Every output is the same from run to run: counts are integers, no sum
 * depends on the order in which threads arrive.  N == 0 or E == 0 returns
 * without touching a device (every R = I, every node its own group, info -1).
 * sfm_last_timings: upload, kernels, download, the consensus kernels alone.
 * ------------------------------------------------------------------- */
int sfm_average_rotations(int32_t n_images, const int32_t *pair_ij, const double *R_rel, const double *weight,
                          int64_t n_edges, uint64_t seed, double threshold, int32_t consensus_sweeps,
                          int32_t max_sweeps, double tol, double *R, double *edge_angle, uint8_t *edge_inlier,
                          int32_t *n_inlier_edges, int32_t *group, int32_t *info, int32_t *level, int32_t *sweeps,
                          int device);

/* ---------------------------------------------------------------------
 * Global rotation averaging with a Gauss-Newton refit solved by conjugate
 * gradients.  Stage 3 of sfm_average_rotations removes a rotation common to
 * all moving nodes by about 1 / (N - 1) per sweep, so its default budget
 * reaches tol only on graphs of about a dozen images; this refit has the same
 * stationary point and moves that common error in one solve: measured, tol
 * 1e-9 is reached in 4 to 5 rounds on graphs of up to 300 images, while at
 * 10,000 images x 500,000 pairs the step falls by 2.5 x per round from the
 * fourth round on and 10 rounds end at 7.8e-8; raise rounds there.
 * Stages 1 and 2, the edge outputs, group, info, level, the gauge and the
 * argument rules are those of sfm_average_rotations, with max_sweeps replaced
 * by rounds >= 0, cg_tol finite and >= 0, cg_max_iters >= 1.  Stage 3 is
 * `rounds` rounds; each takes the current R:
 *   per edge e = (i, j): P = R_rel R_i (the products above), t the trace sum
 *     of P against R_j, a_e = 1 where t >= tau and 0 otherwise -- the trace
 *     test, made again in every round as the Jacobi refit makes it in every
 *     sweep -- and g_e = log(P R_j^T) by stage 3's formulas (M, v, s,
 *     theta = atan2(s, (t - 1) / 2), v theta / s, v where s = 0);
 *   the linearised cost: with R_n <- exp(delta_n) R_n and delta = 0 at every
 *     root, minimise sum_e w_e a_e |g_e + R_rel,e delta_i - delta_j|^2; the
 *     Jacobian of the log is taken as the identity (the residuals lie below
 *     threshold).  The normal equations A delta = b have the 3 x 3 blocks
 *       D_n = (sum of w_e a_e over n's entries) I,
 *       off-diagonal, for j's entry of e: -w_e a_e R_rel; for i's: -w_e a_e R_rel^T,
 *       b_j += w_e a_e g_e and b_i -= w_e a_e R_rel^T g_e,
 *     and the operator is applied from the adjacency as u_e = p_j - R_rel p_i
 *     (a root's p is 0), q_j += w_e a_e u_e, q_i -= w_e a_e R_rel^T u_e, a node's
 *     entries in ascending edge order;
 *   a node without an active entry (D_n = 0) and every root are no unknowns:
 *     their delta is 0 and they keep R;
 *   b = 0 says that sum w log(P R^T) = 0 over each node's passing entries: the
 *     stationary condition of the Jacobi refit, so both refits end at the same
 *     rotations;
 *   a component of the active graph that has lost its root has a gauge
 *     freedom: A is positive semidefinite there, b lies in its range and
 *     conjugate gradients from 0 stay in it (the minimum-norm solution);
 *   the solve, preconditioned by D^-1 (a scalar per node):
 *     x = 0; r = b; z = D^-1 r; p = z; rho = r.z; k = 0;
 *     while k < cg_max_iters and |r| > cg_tol |b|:
 *       q = A p; alpha = rho / p.q; x += alpha p; r -= alpha q; z = D^-1 r;
 *       rho' = r.z; p = z + (rho' / rho) p; rho = rho'; k += 1
 *     cg_iters[round] = k; cg_residual[round] = |r| / |b| (0 where |b| = 0,
 *     with no iteration).  An iteration whose p.q is not > 0 is not made and
 *     ends the solve with x as it is: p has vanished to working precision,
 *     which only cg_tol = 0 (a solve ended by cg_max_iters alone) can reach;
 *   the retraction R_n <- exp(x_n) R_n, the exp of stage 3 with its series
 *     below 1e-4;
 *   step[round] = max_n |x_n|.  The rounds end after the first one with
 *     step <= tol, where tol > 0, or after `rounds`; tol = 0 runs exactly
 *     `rounds`; *sweeps reports the rounds run.
 * New outputs, caller-allocated, `rounds` long each, 0 past the rounds run:
 * cg_iters, cg_residual, step.
 * Device, fp64, 256-thread workgroups: per round one launch over the edges
 * (a_e w_e and g_e, all that is kept per edge) and one in which G lanes per
 * node gather b and D^-1; per CG iteration two launches as in
 * sfm_average_positions' path 2 (the p update fused into the apply, the
 * partial sums added again in a fixed order by every workgroup, the stop a
 * device word that later launches test and the host reads every 8
 * iterations); then the retraction, whose step is an integer maximum over the
 * bits of the doubles.  G (a power of two, 1 .. 64) and the grids come from
 * the graph's size as for position averaging.  No float atomics: two calls
 * give the same bytes.  Sums over a node's entries meet in a tree of G lanes,
 * so results agree with another summation order to rounding, not bitwise.
 * N == 0 or E == 0 returns without touching a device.
 * sfm_last_timings: upload, kernels, download, the CG launches alone.
 * ------------------------------------------------------------------- */
int sfm_average_rotations_cg(int32_t n_images, const int32_t *pair_ij, const double *R_rel, const double *weight,
                             int64_t n_edges, uint64_t seed, double threshold, int32_t consensus_sweeps,
                             int32_t rounds, double tol, double cg_tol, int32_t cg_max_iters, double *R,
                             double *edge_angle, uint8_t *edge_inlier, int32_t *n_inlier_edges, int32_t *group,
                             int32_t *info, int32_t *level, int32_t *sweeps, int32_t *cg_iters, double *cg_residual,
                             double *step, int device);

/* ---------------------------------------------------------------------
 * Global position averaging: the centre of every camera from the directions
 * between the cameras of the pairs, in one call -- rounds of a preconditioned
 * conjugate-gradient solve with reweighting between them.  sfm_init_pairs gives
 * a unit baseline for every verified pair and sfm_average_rotations every
 * camera's rotation; together they give the direction of every pair in world
 * coordinates, and this turns all of them into centres, with an edge mask.  The
 * reference has no counterpart.
 * n_images = N >= 0 cameras; the n_edges = E >= 0 edges are pair_ij (E x 2
 * int32: i != j, both in [0, N); duplicate pairs and both orientations of a
 * pair are allowed, each is an edge of its own) with dir (E x 3 fp64): the
 * direction from C_i towards C_j in world coordinates, finite and not zero; the
 * host divides it by its largest |component| and then by its norm, d_e below is
 * the result.  weight (E, finite and > 0) is nullable: every weight 1.
 * 0 < mu <= 1; sigma finite, > 0, radians; threshold finite, in (0, pi),
 * radians; rounds >= 1; cg_tol finite, >= 0; cg_max_iters >= 1; path 0, 1 or
 * 2; E <= 2^30.  A violation is SFM_ERR_ARG, found on the host before a device
 * is looked for, with nothing written; so is path = 1 with more than
 * SFM_POSITIONS_PATH1_MAX_NODES solved nodes.
 * The graph that is solved (host): a node's entries are the edges that contain
 * it, by ascending edge index.  Nodes with fewer than 2 distinct neighbours are
 * dropped, again and again until none is left: the distance of a leaf along
 * its one direction is undetermined.  Of what remains only the largest
 * connected component (union-find; most nodes, the one with the lowest node on
 * ties) is solved: its M nodes, the "solved" ones, and the edges between them.
 * The root is the solved node with the most entries among those edges, the
 * lowest index on ties.  Parallel rigidity beyond this is not checked; a graph
 * that is not rigid shows as solves that end at cg_max_iters.
 * A round has a weight w_e and a target length s_e per edge; round 0 has
 * w_e = weight_e and s_e = 1.  With v_e = C_j - C_i it minimises
 *   sum_e w_e ( |v_e - d_e (d_e.v_e)|^2 + mu (d_e.v_e - s_e)^2 )
 * over the centres with the root at 0: the linear system A x = b over the
 * other M - 1 nodes with the 3 x 3 blocks
 *   off-diagonal, per entry of n with neighbour m:  -w_e (I - (1 - mu) d_e d_e^T),
 *   diagonal D_n: the sum of w_e (I - (1 - mu) d_e d_e^T) over n's entries,
 *   b_n: the sum over n's entries of +mu w_e s_e d_e where n is the edge's j and
 *        -mu w_e s_e d_e where it is the edge's i.
 * mu = 0 would be the chordal cost, singular on exact data; mu > 0 fixes the
 * scale and bounds the condition number, and since the targets follow the
 * iterate the fixed point carries no length bias.  D_n >= mu (sum w) I is
 * always invertible (by cofactors).
 * A solve: conjugate gradients preconditioned by the D_n^-1, the operator
 * applied from the adjacency as q_n = sum over n's entries of
 * w_e (u - (1 - mu) d_e (d_e.u)), u = p_n - p_m (the root's p is 0):
 *   x = x0 (0 in round 0, then the normalised centres of the round before);
 *   r = b - A x; z = D^-1 r; p = z; rho = r.z; k = 0;
 *   while k < cg_max_iters and |r| > cg_tol |b|:
 *     q = A p; alpha = rho / p.q; x += alpha p; r -= alpha q; z = D^-1 r;
 *     rho' = r.z; p = z + (rho' / rho) p; rho = rho'; k += 1
 *   cg_iters[round] = k; cg_residual[round] = |r| / |b| (0 where |b| = 0).
 * After the solve c = sum_e w_e (d_e.v_e) / sum_e w_e on the round's weights;
 * c not finite or <= 0 ends the call with SFM_ERR_NUMERIC (every output 0, info
 * -1).  Every centre is divided by c, and on the divided centres, per edge:
 *   l = |v_e|; theta_e = atan2(|d_e x v_e|, d_e.v_e);
 *   s_e <- max(d_e.v_e, 1e-3);
 *   w_e <- weight_e / ((1 + (theta_e / sigma)^2) max(l, 1e-3)^2).
 * `rounds` rounds run; the outputs are those of the last solve and its division.
 * Outputs, caller-allocated: C (N x 3), 0 for a node that was not solved;
 * edge_angle (E) = theta_e, edge_length (E) = d_e.v_e, edge_inlier (E) = 1 where
 * theta_e <= threshold -- all three 0 for an edge with an endpoint that was not
 * solved; info (N): 1 the root, 0 another solved node, -1 a node not solved;
 * cg_iters and cg_residual (rounds each); *n_solved = M; *path_used: 1 or 2, 0
 * where no device was used.  Gauge: the root is at 0 and the weighted mean of
 * d_e.v_e is 1, so the scale is arbitrary.  N == 0, E == 0 or M == 0 returns
 * without touching a device.
 * Device, fp64.  path = 1: one workgroup, one launch for all rounds; x, r, p,
 * z, q and the six distinct entries of every D_n^-1 live in LDS, 168 bytes a
 * node, which with the static 64 KB would stop near 390 nodes; with dynamic LDS
 * the bound is SFM_POSITIONS_PATH1_MAX_NODES = 512 solved nodes (86,208 bytes),
 * the root included.  path = 2: any size, two launches per CG iteration and no
 * grid-wide barrier; the stop is tested on the device and read by the host
 * every 8 iterations.  path = 0 takes path 1 where M fits and path 2 otherwise.
 * On either path a node's entries are walked by G lanes (a power of two, 1 ..
 * 64) whose partial sums meet in a fixed tree, and every sum over nodes or edges
 * is a fixed tree too: no float atomics, every output bit-identical from run
 * to run on one path.  The two paths add in different orders, so they agree
 * with each other (and with a dense solve) to a tolerance, not bitwise.
 * sfm_last_timings: upload, kernels, download, the CG iterations alone.
 * ------------------------------------------------------------------- */
#define SFM_POSITIONS_PATH1_MAX_NODES 512
int sfm_average_positions(int32_t n_images, const int32_t *pair_ij, const double *dir, const double *weight,
                          int64_t n_edges, double mu, double sigma, double threshold, int32_t rounds, double cg_tol,
                          int32_t cg_max_iters, int32_t path, double *C, double *edge_angle, uint8_t *edge_inlier,
                          double *edge_length, int32_t *info, int32_t *cg_iters, double *cg_residual,
                          int32_t *n_solved, int32_t *path_used, int device);

/* ---------------------------------------------------------------------
 * Track merging: the rows of a match store that share a keypoint joined into
 * tracks, on the device.  A matching-file line lists only the direct matches
 * of one keypoint of its source image, so one scene point arrives as several
 * rows; this is the track-building step between matching and geometry.  The
 * reference has no counterpart.
 * The n_rows rows are CSR rows of the feature-major store: row r owns
 * observations [row_start[r], row_start[r+1]) of image (0-based), x and y.
 * Definitions, from which every output follows:
 *   keypoint of an observation: the smallest observation index with the same
 *     image and the same x and y as doubles (bit patterns, -0.0 taken as +0.0);
 *   component of a row: the smallest row index reachable from it, two rows
 *     being joined when they contain the same keypoint;
 *   conflicting component: one that contains two different keypoints of one
 *     image (a single row that lists an image twice with different coordinates
 *     is one as well);
 *   label of a row: its component when that is not conflicting; otherwise -1
 *     under SFM_MERGE_DROP and the row's own index under SFM_MERGE_KEEP_ROWS
 *     (the row stays the track it was);
 *   tracks: the distinct non-negative labels, ascending; a track's
 *     observations are the distinct keypoints of the rows that carry its label,
 *     ordered by (image, keypoint index).
 * Outputs, caller-allocated, every one but n_tracks nullable: keypoint (n_obs);
 * component, conflict (1 or 0) and label (n_rows each); *n_tracks; track_label
 * and track_start (room for n_rows and n_rows + 1 entries, the first n_tracks
 * and n_tracks + 1 written); track_obs (room for n_obs keypoint indices, the
 * first track_start[n_tracks] written: track t owns [track_start[t],
 * track_start[t+1])); obs_slot (n_obs): the position in track_obs of the
 * observation's keypoint inside its row's track, -1 for a dropped row.
 * SFM_ERR_ARG, found on the host with nothing written: row_start not starting
 * at 0, decreasing or not ending at n_obs; an image outside [0, n_images); a
 * coordinate that is not finite; an unknown policy; more than 2^30 rows or
 * observations, or bits(n_rows) + bits(n_images) + bits(n_obs) > 64 (the order
 * inside the tracks comes from one 64-bit radix sort).  n_rows == 0 succeeds
 * with no track and n_obs == 0 with one empty track per row, without a device.
 * Integer work throughout: every output is the same from run to run and does
 * not depend on the order in which threads arrive (every choice is a minimum or
 * a sorted order).  No thread waits for another; a conflicting row that is
 * kept is searched linearly for its repeated keypoints, so rows are expected
 * to be short (at most one observation per image in a parsed store).
 * sfm_last_timings: upload, kernels, download.
 * ------------------------------------------------------------------- */
enum { SFM_MERGE_DROP = 0, SFM_MERGE_KEEP_ROWS = 1 };
int sfm_merge_tracks(const int64_t *row_start, int64_t n_rows, const int32_t *image, const double *x,
                     const double *y, int64_t n_obs, int32_t n_images, int32_t policy, int32_t *keypoint,
                     int32_t *component, uint8_t *conflict, int32_t *label, int64_t *n_tracks,
                     int32_t *track_label, int64_t *track_start, int32_t *track_obs, int32_t *obs_slot,
                     int device);

/* ---------------------------------------------------------------------
 * Descriptor matching: image pairs to matches, on the device.  The stage in
 * front of track merging; the reference ships matching files and nothing
 * that produces them.
 * desc is n_kp x dim uint8, row-major (SIFT / RootSIFT descriptors as
 * extractors store them), dim 64, 128 or 256; image k owns the keypoints
 * [img_start[k], img_start[k+1]) (n_images + 1 entries).  pairs is P x 2
 * image numbers (i, j), i != j, in either order; an image may appear in any
 * number of pairs.
 * Definitions, from which every output follows; integer work except one fp64
 * product:
 *   dsq(a, b): the squared Euclidean distance of two descriptors, exact in
 *     int32 (dim * 255^2 < 2^24);
 *   for keypoint a of image i in a pair (i, j), the keypoints of j are ordered
 *     by (dsq, local index): nn is the first of that order and d1 its dsq, d2
 *     the dsq of the second; with fewer than two keypoints in j d2 is
 *     INT32_MAX, with none nn = -1 and d1 = INT32_MAX;
 *   nn_rev of keypoint b of j: the same first-of-order over the keypoints of i;
 *   a is matched to nn when nn >= 0, d1 <= max_dsq (INT32_MAX switches the
 *     test off), d2 == INT32_MAX or (double)d1 < (ratio*ratio) * (double)d2
 *     (ratio*ratio one fp64 product, the right-hand side another), and, with
 *     cross_check, nn_rev[nn] == a.
 * The ratio test applies to the forward direction only, so the matches of
 * (i, j) and of (j, i) may differ.
 * Outputs, caller-allocated: match_start (P + 1): pair p owns
 * [match_start[p], match_start[p+1]) of match_a / match_b (keypoint indices
 * local to image i / j) and match_dsq, `capacity` entries each, the first
 * match_start[P] written; a pair's matches are in ascending a, the pairs in
 * the order given.  capacity must be at least the sum over the pairs of N_i,
 * or of min(N_i, N_j) with cross_check.  Nullable diagnostics, pair-major,
 * never downloaded when null: nn, d1, d2 (sum of N_i entries each) and nn_rev
 * (sum of N_j).
 * SFM_ERR_ARG, found on the host before a device is looked for, with nothing
 * written: a null required pointer; dim not 64, 128 or 256; img_start not
 * starting at 0, decreasing or not ending at n_kp; an image with more than
 * 2^20 keypoints; a pair image outside [0, n_images) or i == j; ratio outside
 * (0, 1] or not finite; max_dsq < 0; cross_check not 0 or 1; capacity below
 * the bound.  P == 0 succeeds without a device.
 * Every output is the same from run to run (integer minima and a scan).
 * sfm_last_timings: upload, kernels, download.
 * ------------------------------------------------------------------- */
int sfm_match_descriptors(const uint8_t *desc, int64_t n_kp, const int64_t *img_start, int32_t n_images, int32_t dim,
                          const int32_t *pairs, int64_t P, double ratio, int32_t max_dsq, int32_t cross_check,
                          int64_t capacity, int64_t *match_start, int32_t *match_a, int32_t *match_b,
                          int32_t *match_dsq, int32_t *nn, int32_t *d1, int32_t *d2, int32_t *nn_rev, int device);

/* ---------------------------------------------------------------------
 * Guided descriptor matching: sfm_match_descriptors with the candidates of a
 * keypoint restricted to a band around its epipolar line.  The stage behind
 * pair verification: with a trusted F per pair, the matches that the ratio
 * test and the cross-check lose to repeated structure come back.
 * The arguments of sfm_match_descriptors and: xy, n_kp x 2 fp64 keypoint
 * coordinates in desc's row order; F, P x 9 fp64 row-major, one matrix per
 * pair in sfm_verify_pairs' convention x_j^T F x_i = 0 for the pair (i, j)
 * -- (x, y) is the keypoint of the first image of the pair, (u, v) of the
 * second, and a caller who lists the pair as (j, i) passes F^T; gate, the
 * half-width of the band in pixels, finite and >= 0.
 * Definitions, from which every output follows:
 *   thr2 = gate * gate, one fp64 product; it may overflow to +inf, which is
 *     defined: every pair of keypoints with den > 0 then passes;
 *   gate_p(a, b) for keypoint a = (x, y) of i and b = (u, v) of j under
 *     F = F_p, fp64 with no contraction, in this order of operations:
 *       l0 = (F0 x + F1 y) + F2, l1 = (F3 x + F4 y) + F5, l2 = (F6 x + F7 y) + F8,
 *       m0 = (F0 u + F3 v) + F6, m1 = (F1 u + F4 v) + F7,
 *       e = (u l0 + v l1) + l2, den = (l0 l0 + l1 l1) + (m0 m0 + m1 m1),
 *       gate_p = den > 0 && e e < thr2 den
 *     -- the squared Sampson distance against the squared half-width, the
 *     inlier rule of sfm_verify_pairs bit for bit; false for anything not
 *     finite, so a pair whose F holds a NaN (what sfm_verify_pairs returns for
 *     a failed pair) has no candidates and no matches, which is not an error;
 *   the candidates of a: C(a) = { b in j : gate_p(a, b) }, n_cand[a] = |C(a)|;
 *   nn, d1, d2: sfm_match_descriptors' with the (dsq, local index) order taken
 *     over C(a) only; d2 = INT32_MAX when |C(a)| < 2, nn = -1 and
 *     d1 = INT32_MAX when C(a) is empty;
 *   nn_rev[b]: the first of the same order over { a in i : gate_p(a, b) } --
 *     the same predicate with the same argument roles and the same bits, no
 *     transposed matrix, so a pair of keypoints is a candidate in both
 *     directions or in neither;
 *   acceptance (max_dsq, the ratio test on the forward direction only,
 *     cross_check), compaction, the capacity bound, the pair-major order and
 *     ascending a inside a pair are sfm_match_descriptors'.
 * Outputs as sfm_match_descriptors'; n_cand is one more nullable diagnostic,
 * pair-major like nn (sum of N_i entries).
 * SFM_ERR_ARG, found on the host before a device is looked for, with nothing
 * written: everything sfm_match_descriptors refuses; a null xy with n_kp > 0;
 * a null F with P > 0; gate negative or not finite.  P == 0 succeeds without
 * a device.
 * Every output is the same from run to run.
 * sfm_last_timings: upload, kernels, download.
 * ------------------------------------------------------------------- */
int sfm_match_descriptors_guided(const uint8_t *desc, const double *xy, int64_t n_kp, const int64_t *img_start,
                                 int32_t n_images, int32_t dim, const int32_t *pairs, const double *F, int64_t P,
                                 double gate, double ratio, int32_t max_dsq, int32_t cross_check, int64_t capacity,
                                 int64_t *match_start, int32_t *match_a, int32_t *match_b, int32_t *match_dsq,
                                 int32_t *nn, int32_t *d1, int32_t *d2, int32_t *nn_rev, int32_t *n_cand, int device);

/* ---------------------------------------------------------------------
 * Feature extraction: images to keypoints and descriptors, on the device.
 * The stage in front of sfm_match_descriptors: a difference-of-Gaussians
 * (DoG) detector after Lowe with the 128-byte gradient-histogram descriptor
 * that sfm_match_descriptors takes.  The reference has no extractor.
 * images is n_images x H x W uint8, row-major greyscale, all of one size.
 * n_octaves == 0 means as many octaves as keep the smaller side >= 16.
 * Definitions, from which every output follows; fp32 unless stated:
 *   pixels are u8 / 255.  Octave 0 has the input's size (no up-sampling);
 *     S = 3: an octave has S + 3 Gaussian layers and S + 2 DoG layers; layer
 *     l carries sigma_l = sigma 2^(l/S).  The input is taken to carry blur
 *     0.5: layer 0 of octave 0 is the input blurred by sqrt(sigma^2 - 0.25),
 *     layer l > 0 is layer l - 1 blurred by sqrt(sigma_l^2 - sigma_(l-1)^2);
 *     layer 0 of a later octave is every second pixel (0, 2, 4, ..) of layer
 *     S of the octave before, so an octave of h x w is followed by one of
 *     ceil(h/2) x ceil(w/2).
 *   a blur of s is separable, rows then columns, radius R = ceil(4 s), the
 *     2R + 1 taps exp(-i^2 / (2 s^2)) computed in fp64, normalised to sum 1,
 *     then rounded to fp32; borders reflect-101; each output one fp32 sum.
 *   D_l = G_(l+1) - G_l, one fp32 subtraction.
 *   a candidate is a pixel (r, c) of D_l, 1 <= l <= S, 5 <= r < h - 5,
 *     5 <= c < w - 5, with |D| > fp32(0.5 contrast_threshold / S) and D
 *     strictly greater, or strictly smaller, than all 26 neighbours.
 *   refinement: with the gradient g and the Hessian Hs of D by central
 *     differences at (l, r, c), the offset X = (xc, xr, xs) solves Hs X = -g
 *     (adjugate over determinant; rejected when the determinant is 0 or not
 *     finite or a component reaches 1000).  While a component exceeds 0.5 in
 *     magnitude the site moves by floor(X + 0.5), at most 5 times; rejected
 *     when the sixth solve still exceeds 0.5, or the site leaves 1 <= l <= S
 *     or the border of 5.  D^ = D + 0.5 g.X; rejected when |D^| S <
 *     contrast_threshold, or when the 2 x 2 Hessian has det <= 0 or
 *     tr^2 r >= (r + 1)^2 det with r = edge_threshold.
 *     x = (c + xc) 2^octave, y = (r + xr) 2^octave (fp64 of the fp32 offsets;
 *     pixel centres at integers of the input image), scale =
 *     sigma 2^octave 2^((l + xs)/S), response = |D^|.
 *   orientation: sigma_o = sigma 2^((l + xs)/S); over the pixels (r + i,
 *     c + j), |i|, |j| <= floor(4.5 sigma_o + 0.5), strictly inside the layer
 *     G_l, the gradient (G[y][x+1] - G[y][x-1], G[y+1][x] - G[y-1][x]) adds
 *     its magnitude times exp(-(i^2 + j^2) / (2 (1.5 sigma_o)^2)) to bin
 *     floor(36 atan2(dy, dx) / 2 pi + 0.5) mod 36 (angles in [0, 2 pi), from
 *     +x towards +y).  The histogram is smoothed twice by the circular
 *     [1 4 6 4 1] / 16.  Every bin above both neighbours and >= 0.8 of the
 *     maximum gives a keypoint with angle (b + 0.5 (lo - hi) / (lo - 2 h +
 *     hi)) 2 pi / 36 wrapped into [0, 2 pi), in radians.
 *   descriptor: with (xo, yo) = (x, y) / 2^octave, hw = 3 scale / 2^octave,
 *     every pixel of G_l strictly inside the layer and within
 *     floor(hw 3.5355339 + 0.5) + 1 of (floor(xo + 0.5), floor(yo + 0.5)) is
 *     rotated by -angle and divided by hw into (rx, ry); it contributes when
 *     rx + 1.5 and ry + 1.5 lie in (-1, 4): its gradient magnitude times
 *     exp(-(rx^2 + ry^2) / 8) is spread trilinearly over row ry + 1.5, column
 *     rx + 1.5 and orientation bin 8 (atan2(gy, gx) - angle) / 2 pi mod 8;
 *     entry ((row 4) + column) 8 + bin of 128.  L2-normalise, clamp at 0.2,
 *     normalise again; byte = min(255, floor(512 v + 0.5)).
 *   order: an image's keypoints are sorted by (octave, layer, row, column) of
 *     the candidate they come from, then by orientation bin.  With
 *     max_keypoints > 0 only the max_keypoints largest responses of an image
 *     are kept, ties to the smaller key, emitted in key order.
 * Outputs, caller-allocated, n_images x capacity rows each: image k owns rows
 * [kp_start[k], kp_start[k+1]) (kp_start has n_images + 1 entries) of xy (fp64
 * x, y), scale, angle, response (fp32) and desc (128 uint8).  An image with
 * more than `capacity` keypoints (only possible with max_keypoints == 0) ends
 * the call with SFM_ERR_CAPACITY and a message that names the image and its
 * count; nothing is written out of bounds.  So does a cand_capacity below the
 * candidates found.  Both are found while the chunks are processed: kp_start,
 * the outputs and the diagnostics of the images of earlier chunks have been
 * written by then and are valid, those of later images are not.
 * Nullable diagnostics, never downloaded when null: kp_site (4 int32 per
 * keypoint: octave, layer, row, col of the refined site); pyramid (per image
 * the octaves, per octave the S + 3 layers, row-major fp32); and, together,
 * cand_start (n_images + 1), cand (5 int32 per candidate: image, octave,
 * layer, row, col, sorted), ref_ok, ref_site (3 int32: the final layer, row,
 * col) and ref_val (4 fp32: xc, xr, xs, |D^|) per candidate, zero where
 * rejected; cand_capacity is the rows they hold in total.
 * SFM_ERR_ARG, found on the host before a device is looked for, with nothing
 * written: a null required pointer; H or W below 16 or above 65536 (the
 * candidate key's 17 bits); n_octaves < 0 or above the maximum for the size; a
 * threshold or sigma that is not finite or not positive; sigma <= 0.5 (the
 * input's assumed blur) or above 3.2 (a blur radius above 25, the tile the
 * blur kernel's LDS is laid out for: a limit of this implementation, not of
 * the algorithm); max_keypoints < 0; capacity below max_keypoints.
 * n_images == 0 succeeds without a device.
 * The images are processed in chunks; the workspace does not grow with
 * n_images.  Every output is the same from run to run.
 * sfm_last_timings: upload, kernels, download, the pyramid kernels (blurs
 * and down-samples) alone; each summed over the chunks.
 * ------------------------------------------------------------------- */
int sfm_extract_features(const uint8_t *images, int32_t n_images, int32_t H, int32_t W, int32_t n_octaves,
                         int32_t max_keypoints, double contrast_threshold, double edge_threshold, double sigma,
                         int64_t capacity, int64_t *kp_start, double *xy, float *scale, float *angle, float *response,
                         uint8_t *desc, int32_t *kp_site, float *pyramid, int64_t cand_capacity, int64_t *cand_start,
                         int32_t *cand, uint8_t *ref_ok, int32_t *ref_site, float *ref_val, int device);

/* ---------------------------------------------------------------------
 * Visual vocabulary: k-means on uint8 descriptors with uint8 centres, on the
 * device; with max_iterations == 0 the quantisation of descriptors against a
 * given vocabulary.  With sfm_select_pairs the stage that chooses the image
 * pairs sfm_match_descriptors is given; the reference has no such stage.
 * desc is n x dim uint8, row-major, dim 64, 128 or 256; centres is
 * n_words x dim uint8, on entry the initial centres, on return the final ones.
 * Definitions, from which every output follows; everything is integer:
 *   dsq: sfm_match_descriptors' squared distance, exact in int32;
 *   word_t[a]: the first centre of the (dsq, centre index) order over
 *     centres_t;
 *   cnt_t[w]: the number of members of centre w (the a with word_t[a] == w);
 *   sum_t[w][k]: the exact integer sum of byte k over the members of w;
 *   centres_(t+1)[w][k] = floor((2 sum_t[w][k] + cnt_t[w]) / (2 cnt_t[w]))
 *     when cnt_t[w] > 0 -- the mean rounded half up -- and centres_t[w][k]
 *     otherwise: an empty cluster keeps its centre;
 *   inertia[t] = the sum over a of dsq(a, centres_t[word_t[a]]), as int64;
 *   updates run for t = 1, 2, ...: the loop stops after update T when
 *     T == max_iterations or when update T changed no byte; *iterations = T.
 * Outputs, caller-allocated: centres_T, word_T (n, nullable), cnt_T (count,
 * n_words, nullable), inertia[0 .. T] (max_iterations + 1 entries, nullable;
 * entries past T are not written) and *iterations.
 * SFM_ERR_ARG, found on the host before a device is looked for, with nothing
 * written: a null required pointer; dim not 64, 128 or 256; n < 1; n_words
 * < 1, above n or above 2^20; max_iterations < 0; and n above 2^24 with
 * max_iterations > 0 -- the byte sums are 32-bit (255 * 2^24 < 2^32), a limit
 * of this implementation; quantisation (max_iterations == 0) has no such
 * limit.
 * Every output is the same from run to run (integer minima and integer
 * atomics, which are order-independent).
 * sfm_last_timings: upload, kernels, download.
 * ------------------------------------------------------------------- */
int sfm_vocab_train(const uint8_t *desc, int64_t n, int32_t dim, int32_t n_words, int32_t max_iterations,
                    uint8_t *centres, int32_t *word, int64_t *count, int64_t *inertia, int32_t *iterations,
                    int device);

/* ---------------------------------------------------------------------
 * Pair selection: tf-idf retrieval over quantised words, the top_k
 * neighbours of every image.  word is n_kp int32 in [0, n_words) (what
 * sfm_vocab_train returns); image k owns the keypoints
 * [img_start[k], img_start[k+1]) (n_images + 1 entries).
 * Definitions, from which every output follows; integer work except the
 * score:
 *   h[i][w]: the number of keypoints of image i with word w;
 *   df[w]: the number of images with h[i][w] > 0;
 *   q[d] = floor(256 log((double)n_images / (double)d) + 0.5) for
 *     1 <= d <= n_images, a table the host computes with the C library's log
 *     (the device never calls log); a word in every image weighs 0;
 *   v[i][w] = h[i][w] q[df[w]];
 *   norm2[i] = the sum over w of v[i][w]^2 and dot(i, j) = the sum over w of
 *     v[i][w] v[j][w], both exact in int64;
 *   score(i, j) = (double)dot / (sqrt((double)norm2[i]) sqrt((double)norm2[j])):
 *     five IEEE fp64 operations in this order;
 *   the candidates of i are the j != i with dot(i, j) > 0, ordered by score
 *     descending and then by j ascending.
 * Outputs, caller-allocated: row i of neighbour, score and dot (nullable)
 * (n_images x top_k each) holds the first top_k candidates of i, padded with
 * -1, 0.0 and 0; norm2 (n_images) and df (n_words) are nullable.
 * SFM_ERR_ARG, found on the host before a device is looked for, with nothing
 * written: a null required pointer; img_start not starting at 0, decreasing
 * or not ending at n_kp; a word outside [0, n_words); an image with more than
 * 2^18 keypoints; n_images above 16,384; n_words outside [1, 2^20];
 * top_k < 0.  The two limits are limits of this implementation: they keep dot
 * inside int64 (q < 2^12, so q^2 N_i N_j < 2^24 2^36) and let a query's row of
 * int64 accumulators fit in the 160 KB of LDS (16,384 x 8 B = 128 KB).
 * n_images == 0 or top_k == 0 succeeds without a device, with nothing
 * written; so does n_kp == 0, with every row padding, norm2 and df zero.
 * Every output is the same from run to run.
 * sfm_last_timings: upload, kernels, download.
 * ------------------------------------------------------------------- */
int sfm_select_pairs(const int32_t *word, int64_t n_kp, const int64_t *img_start, int32_t n_images,
                     int32_t n_words, int32_t top_k, int32_t *neighbour, double *score, int64_t *dot,
                     int64_t *norm2, int32_t *df, int device);

/* ---------------------------------------------------------------------
 * BundleAdjustment (BundleAdjustment.py:8-242)
 * Camera parameters are the reference's: [rotvec(3), t(3)] with
 * x_cam = R(rotvec) X + t, proj = K x_cam [:2] / (K x_cam [2] + 1e-8),
 * residual r = obs - proj (BundleAdjustment.py:73-110).
 * ------------------------------------------------------------------- */
/* project_points (BundleAdjustment.py:8-40) for one camera P = K[R|-RC]:
 * P is 3 x 4, X is M x 3, out M x 2. */
int sfm_project_points(const double *P, const double *X, int64_t M, double *out, int device);
/* bundle_adjustment_residuals: r (2 * n_obs), interleaved [rx0, ry0, ...]. */
int sfm_ba_residuals(int32_t n_cams, int64_t n_pts, int64_t n_obs, const int32_t *cam_idx,
                     const int32_t *pt_idx, const double *obs, const double *K,
                     const double *cam_params, const double *points, double *r, int device);

typedef struct {
    int32_t max_iterations;      /* LM iterations (damped solve + trial)        */
    int32_t fixed_iterations;    /* 1: run exactly max_iterations (benchmark)   */
    double function_tolerance;   /* stop: accepted step with dcost < ftol*cost  */
    double gradient_tolerance;   /* stop after a linearisation when max |J^T r| < gtol
                                    (status 2; 0 = off; < 0 is SFM_ERR_ARG)      */
    double parameter_tolerance;  /* stop: |dx| < xtol (|x| + xtol)               */
    double initial_lambda;       /* Marquardt damping on clamp(diag(J^T J))      */
} sfm_ba_opts;

typedef struct {
    int32_t iterations;  /* LM iterations performed                             */
    int32_t accepted;    /* accepted steps (re-linearisations)                  */
    int32_t status;      /* 1 ftol, 2 gtol, 3 xtol, 4 max_iterations, 5 lambda,
                            6 cost at x0 not finite (no step taken)             */
    int32_t n_ranks;
    double cost0, cost;  /* 0.5 sum r^2 before / after                          */
    double t_setup_ms;   /* host prep + uploads                                 */
    double t_loop_ms;    /* LM loop wall time                                   */
    double t_download_ms;
    double lambda;
} sfm_ba_report;

/* Observations must be point-major (sorted by pt_idx, as the reference
 * assembles them: BundleAdjustment.py:164-169).  cam_params (n_cams x 6)
 * and points (n_pts x 3) are updated in place.
 * SFM_ERR_ARG, with nothing touched: a camera or point index out of range,
 * observations not point-major, a point observed twice by the same camera,
 * more than 682 cameras, and an empty problem (n_pts == 0 or n_obs == 0:
 * nothing to adjust).  Points and cameras without observations are allowed
 * and do not move.  Within a communicator a rank's shard may be empty. */
int sfm_ba_lm(int32_t n_cams, int64_t n_pts, int64_t n_obs, const int32_t *cam_idx,
              const int32_t *pt_idx, const double *obs, const double *K, double *cam_params,
              double *points, const sfm_ba_opts *opts, sfm_ba_report *report, int device);

/* sfm_ba_lm with the observations of a dense scan (sfm_dense_obs_scan's
 * handle, not freed here; its rows are the n_pts points, its cameras at
 * most n_cams): perform_bundle_adjustment's whole path
 * (BundleAdjustment.py:156-242) from the dense matrices, the observations
 * copied from the scan straight into the pinned upload buffer. */
int sfm_ba_lm_dense(void *obs_handle, int32_t n_cams, int64_t n_pts, const double *K, double *cam_params,
                    double *points, const sfm_ba_opts *opts, sfm_ba_report *report, int device);

/* ---- device-resident BA session (bench / multi-GPU) -------------------
 * A problem is uploaded once and iterated many times.  With a communicator
 * each rank holds a disjoint subset of the points (and all of their
 * observations) and every camera; one RCCL all-reduce (sum, fp64) of the
 * partial reduced camera system per LM iteration + one of the trial cost. */
typedef struct sfm_comm sfm_comm;
typedef struct sfm_ba_problem sfm_ba_problem;

int sfm_comm_unique_id(char out[128]);
int sfm_comm_init(const char id[128], int nranks, int rank, int device, sfm_comm **out);
/* in-process group of nranks communicators (one host thread per rank, any
 * devices, the same device allowed): out receives nranks handles */
int sfm_comm_init_local(int nranks, sfm_comm **out);
int sfm_comm_destroy(sfm_comm *comm);

/* ---- hypothesis-sharded RANSAC: the loop of
 * GetInliersRANSAC.py:53-92 (and GetHomographyInliers.py:124-156) split into
 * contiguous hypothesis ranges [h0, h1), one per rank.
 * Shard key = (count << 32) | (0xFFFFFFFF - iteration), 0 when no hypothesis
 * of the shard has an inlier: the max over ranks is the reference's winner
 * (max count, earliest iteration: the strict '>' update at :85-88).
 * _pyrandom_range draws ALL H rows from the CPython MT19937 state st[625]
 * (in/out) in the reference's order, so st ends where the unsharded call
 * leaves it, and fits/scores only [h0, h1).  counts_out: h1 - h0 entries
 * (nullable).  F_best/H_best: the shard winner's model (untouched when the
 * key is 0).  Requires H < 2^32. */
int sfm_ransac_f8_range(const double *x1, const double *x2, int64_t N, const int32_t *samples /* H x 8 */,
                        int64_t H, int64_t h0, int64_t h1, double thr, int32_t *counts_out,
                        uint64_t *best_key, double *F_best, int device);
int sfm_ransac_f8_pyrandom_range(const double *x1, const double *x2, int64_t N, uint32_t *st, int64_t H,
                                 int64_t h0, int64_t h1, double thr, int32_t *counts_out,
                                 uint64_t *best_key, double *F_best, int device);
int sfm_ransac_h4_pyrandom_range(const double *x1, const double *x2, int64_t N, uint32_t *st, int64_t H,
                                 int64_t h0, int64_t h1, double thr, int32_t *counts_out,
                                 uint64_t *best_key, double *H_best, int device);
/* max of the ranks' keys (in/out) and the winner's model (in/out, 9) over
 * comm: RCCL all-reduce(max, u64) then a sum in which only the winner
 * contributes; or the in-process group.  Every rank returns the same. */
int sfm_ransac_combine(sfm_comm *comm, uint64_t *key, double *model);
/* inlier mask of one model (GetInliersRANSAC.py:67-81 /
 * GetHomographyInliers.py:135-146): the winner's emit after the combine */
int sfm_ransac_f8_mask(const double *x1, const double *x2, int64_t N, const double *F, double thr,
                       uint8_t *mask, int device);
int sfm_ransac_h4_mask(const double *x1, const double *x2, int64_t N, const double *Hm, double thr,
                       uint8_t *mask, int device);

int sfm_ba_create(int32_t n_cams, int64_t n_pts, int64_t n_obs, const int32_t *cam_idx,
                  const int32_t *pt_idx, const double *obs, const double *K,
                  const double *cam_params, const double *points, int device, sfm_comm *comm,
                  sfm_ba_problem **out);
int sfm_ba_solve(sfm_ba_problem *p, const sfm_ba_opts *opts, sfm_ba_report *report);
/* digest of the Schur sweep plan built at create (set only when the
 * environment has SFM_PLAN_DIGEST=1, else 0): the device planner and the
 * host planner (SFM_PLAN_HOST=1) must produce the same plan */
int sfm_ba_plan_digest(sfm_ba_problem *p, uint64_t *out);
/* the speculative sweep's dispatch (the rejection branch's Schur system built
 * beside the reduced solve): out = {free CUs, whole (spec, range) items,
 * split specs, sub-ranges per split item (0: no split)}; all 0 when the
 * problem cannot speculate (several ranks, the Cholesky fallback) */
int sfm_ba_spec_plan(sfm_ba_problem *p, int32_t out[4]);
/* reset the device state to the initial parameters given at create time */
int sfm_ba_reset(sfm_ba_problem *p);
int sfm_ba_download(sfm_ba_problem *p, double *cam_params, double *points);
/* per-phase HIP events in the following solves (off by default: each event
 * record costs the stream a few microseconds) */
int sfm_ba_set_timing(sfm_ba_problem *p, int on);
/* average device time per LM iteration of each kernel family over the
 * last solve with timing on (ms; zeros otherwise): names are written
 * ';'-separated into `names`. */
int sfm_ba_kernel_times(sfm_ba_problem *p, double *ms, int n, char *names, int names_len);
/* Diagnostic: x = S^-1 rhs for an SPD n x n S (row-major) with the reduced
 * camera system solver of sfm_ba_solve (the scipy 'lm' reference solves the
 * same normal equations inside least_squares, BundleAdjustment.py:205-213).
 * SFM_ERR_SOLVE if a pivot is not positive. */
int sfm_reduced_solve(const double *S, const double *rhs, int32_t n, double *x, int device);
int sfm_ba_destroy(sfm_ba_problem *p);

/* single-process multi-GPU BA: points split over `devices` (n_ranks
 * entries; repeats allowed), one host thread per rank, reduced camera
 * system summed every LM iteration.  Same arguments as sfm_ba_lm. */
int sfm_ba_lm_multi(int32_t n_cams, int64_t n_pts, int64_t n_obs, const int32_t *cam_idx,
                    const int32_t *pt_idx, const double *obs, const double *K, double *cam_params,
                    double *points, const sfm_ba_opts *opts, sfm_ba_report *report, const int *devices,
                    int n_ranks);

#ifdef __cplusplus
}
#endif
#endif /* SFMCORE_H */

"""Multi-view track triangulation from the COO store: one point per feature
from ALL of its views among the registered cameras, in one device call.

The reference's registration loop (Wrapper_dev.py:262-291) triangulates a new
image against every earlier one, a pair at a time, and writes each pair's
points over the last, so a feature seen in five images keeps the point of
two of them.  ``triangulate_store`` differs on purpose: every flagged
observation of a track enters the N-view DLT and the refinement
(``sfm_triangulate_tracks``), with one upload of the observations.

``triangulate_store_robust`` is the step between that and bundle adjustment:
tracks built from pairwise matches hold wrong observations, and the bundle
adjuster has no robust loss.  It fits every track to the observations that
agree (``sfm_triangulate_tracks_robust``), says which tracks to keep and can
clear the store's flags of everything else.

``verify_pairs`` is the stage before all of them: F-RANSAC for every image pair
of the store in one call (``sfm_verify_pairs``), which sets the flags the others
read.  ``init_pairs`` follows it: the pose, cheirality, parallax and
homography support of every verified pair in one call (``sfm_init_pairs``), and
from them the pair to start the reconstruction from.

``pair_rotations`` and ``average_rotations`` use what ``init_pairs`` computes
for every pair and the incremental chain then drops: all cameras' rotations at
once from the relative rotations (``sfm_average_rotations``), with the mask of
the pairs that are consistent around the loops of the view graph.

``pair_directions`` and ``average_positions`` are the other half of that global
path: the pairs' baselines turned into world directions by the averaged
rotations, and all camera centres at once from them
(``sfm_average_positions``), so that triangulation and bundle adjustment can
start with every camera.

``merge_tracks`` comes before every one of them, right after read_matching: the
store's rows that share a keypoint joined into tracks on the device
(``sfm_merge_tracks``; sfm_io.merge_tracks, also MatchStore.merge_tracks).
"""
import numpy as np

import _sfmcore as _core
from sfm_io import merge_tracks  # noqa: F401  (the stage list's first entry lives with the store)
from sfm_io import extract_features  # noqa: F401  (the first stage: images to keypoints and descriptors)
from sfm_io import train_vocabulary, quantize, select_pairs  # noqa: F401  (which pairs to match: retrieval)
from sfm_io import match_descriptors  # noqa: F401  (in front of it: descriptors to a store)
from sfm_io import match_descriptors_guided  # noqa: F401  (behind verify_pairs: rematch_verified)
from sfm_two_view import projection


def triangulate_store(store, K, C_set, R_set, images=None, refine=True):
    """Tracks of ``store`` (a MatchStore) over ``images`` (default
    range(len(C_set))), camera i of C_set / R_set belonging to images[i].
    Returns (feature_rows, X, cost, front, info): the feature row of each
    track and ``_sfmcore.triangulate_tracks``'s outputs for it."""
    images = np.arange(len(C_set)) if images is None else np.asarray(images)
    if len(images) != len(C_set) or len(R_set) != len(C_set):
        raise ValueError("triangulate_store: one C and one R per image")
    K = np.asarray(K, dtype=np.float64)
    P = np.stack([projection(K, np.asarray(C, dtype=np.float64).reshape(3), np.asarray(R, dtype=np.float64))
                  for C, R in zip(C_set, R_set)]) if len(C_set) else np.zeros((0, 3, 4))
    feature_rows, track_start, obs_cam, obs_xy = store.tracks(images)
    X, cost, front, info = _core.triangulate_tracks(P, track_start, obs_cam, obs_xy, refine=refine)
    return feature_rows, X, cost, front, info


def triangulate_store_robust(store, K, C_set, R_set, images=None, threshold=4.0, min_inliers=3, min_angle_deg=0.0,
                             update_flags=False):
    """Robust ``triangulate_store``: the tracks of ``store`` over ``images``,
    each fitted to its inlier observations (within ``threshold`` pixels).
    Returns (feature_rows, out, keep): ``out`` is
    ``_sfmcore.triangulate_tracks_robust``'s tuple (X, cost, n_inliers,
    inlier, best_pair, best_count, info, angle), angle from C_set; ``keep``
    (T,) bool marks the tracks with info >= 1, n_inliers >= min_inliers and
    angle >= min_angle_deg.  With ``update_flags`` the store's flag is set to
    0 for every outlier observation of a kept track and for every observation
    of a dropped one, so that ``MatchStore.observations`` -- and the bundle
    adjustment fed from it -- no longer sees them."""
    images = np.arange(len(C_set)) if images is None else np.asarray(images)
    if len(images) != len(C_set) or len(R_set) != len(C_set):
        raise ValueError("triangulate_store_robust: one C and one R per image")
    K = np.asarray(K, dtype=np.float64)
    centres = np.array([np.asarray(C, dtype=np.float64).reshape(3) for C in C_set]).reshape(-1, 3)
    P = np.stack([projection(K, C, np.asarray(R, dtype=np.float64)) for C, R in zip(centres, R_set)]) \
        if len(C_set) else np.zeros((0, 3, 4))
    feature_rows, track_start, obs_cam, obs_xy, index = store.tracks(images, return_index=True)
    out = _core.triangulate_tracks_robust(P, track_start, obs_cam, obs_xy, threshold=threshold,
                                          min_inliers=min_inliers, centres=centres)
    keep = robust_keep(out, min_inliers, min_angle_deg)
    if update_flags:
        clear_outlier_flags(store, track_start, index, out[3], keep)
    return feature_rows, out, keep


def register_views(store, K, feature_rows, X, candidates, H=256, seed=0, threshold=4.0, min_inliers=6,
                   update_flags=False):
    """Which image to register next, and with what pose: every image of
    ``candidates`` against the points X (row i belongs to feature_rows[i]) in
    one device call (``_sfmcore.register_views``: 6-point PnP RANSAC over H
    hypotheses per view, pose refit, inlier mask).  It replaces the
    reference's per-image PnPRANSAC + NonlinearPnP (Wrapper_dev.py:232-249).
    Returns (order, out, index): ``out`` is ``_sfmcore.register_views``'s tuple
    (C, R, cost, n_inliers, inlier, best_hyp, best_count, info) over the CSR
    correspondences of ``store.correspondences(feature_rows, candidates)``,
    ``index`` their store indices, ``order`` the candidates by decreasing
    n_inliers (stable), so candidates[order[0]] is the next best view.  With
    ``update_flags`` the store's flag is set to 0 for the outlier
    observations of every view with info >= 1."""
    view_start, pt_idx, xy, index = store.correspondences(feature_rows, candidates)
    samples = _core.register_samples(np.diff(view_start), H, seed)
    out = _core.register_views(K, X, view_start, pt_idx, xy, samples, threshold=threshold, min_inliers=min_inliers)
    order = np.argsort(-out[3].astype(np.int64), kind="stable")
    if update_flags:
        registered = np.repeat(out[7] >= 1, np.diff(view_start))
        store.flag[index[registered & ~out[4]]] = 0
    return order, out, index


def register_views_p3p(store, K, feature_rows, X, candidates, H=256, seed=0, threshold=4.0, min_inliers=4,
                       update_flags=False):
    """``register_views`` with the calibrated minimal solver
    (``_sfmcore.register_views_p3p``: P3P RANSAC over H 3-point samples per
    view, up to four poses per sample).  Use it where K is trusted: it needs
    half the points per sample and registers views of points on one plane,
    which the 6-point DLT cannot.  Same arguments, same (order, out, index)
    with the same meaning; code that consumes ``register_views`` works on it
    unchanged."""
    view_start, pt_idx, xy, index = store.correspondences(feature_rows, candidates)
    samples = _core.p3p_samples(np.diff(view_start), H, seed)
    out = _core.register_views_p3p(K, X, view_start, pt_idx, xy, samples, threshold=threshold,
                                   min_inliers=min_inliers)
    order = np.argsort(-out[3].astype(np.int64), kind="stable")
    if update_flags:
        registered = np.repeat(out[7] >= 1, np.diff(view_start))
        store.flag[index[registered & ~out[4]]] = 0
    return order, out, index


def verify_pairs(store, images=None, H=256, seed=0, threshold=2.5, min_inliers=8, min_matches=8,
                 update_flags=False):
    """The first stage of the pipeline: the epipolar geometry of every image
    pair of ``store`` over ``images`` (default all) in one device call
    (``_sfmcore.verify_pairs``: 8-point F-RANSAC over H hypotheses per pair
    under x2^T F x1 = 0, the Sampson distance as the inlier rule, a
    least-squares refit on the consensus set, one inlier mask per
    correspondence).  It replaces the reference's pair loop
    (Wrapper_dev.py:69-123), whose F does not fit its own sample points.
    Returns (order, pair_ij, out, index1, index2): ``pair_ij`` (P, 2) and the
    store indices ``index1`` / ``index2`` of every correspondence's two
    observations are ``store.pairs(images, min_matches)``'s, ``out`` is
    ``_sfmcore.verify_pairs``'s tuple (F, cost, n_inliers, inlier, best_hyp,
    best_count, info) over them, ``order`` the pairs by decreasing n_inliers
    (stable), so pair_ij[order[0]] is the candidate initial pair.  With
    ``update_flags`` the store's flag is set to 1 for both observations of
    every inlier correspondence of every pair with info >= 0 -- what
    Wrapper_dev.py:122-123 does to filtered_feature_flags; no flag is cleared."""
    pair_ij, pair_start, index1, index2 = store.pairs(images, min_matches=min_matches)
    x1 = np.column_stack([store.x[index1], store.y[index1]])
    x2 = np.column_stack([store.x[index2], store.y[index2]])
    samples = _core.pair_samples(np.diff(pair_start), H, seed)
    out = _core.verify_pairs(pair_start, x1, x2, samples, threshold=threshold, min_inliers=min_inliers)
    order = np.argsort(-out[2].astype(np.int64), kind="stable")
    if update_flags:
        ok = np.repeat(out[6] >= 0, np.diff(pair_start)) & out[3]
        store.flag[index1[ok]] = 1
        store.flag[index2[ok]] = 1
    return order, pair_ij, out, index1, index2


def verify_pairs_calibrated(store, K, images=None, H=256, seed=0, threshold=2.5, min_inliers=8, min_matches=8,
                            update_flags=False):
    """``verify_pairs`` with the calibration: the essential matrix of every
    image pair of ``store`` over ``images`` (default all) in one device call
    (``_sfmcore.essential_pairs``: 5-point RANSAC over H hypotheses per pair,
    scored in pixels by the Sampson distance of F = K^-T E K^-1, the winner
    refitted as E = [t]x R on its consensus set).  Unlike the 8-point F it has a
    model for a pair that looks at one plane, and its E is an essential matrix.
    Returns (order, pair_ij, out, index1, index2) with ``verify_pairs``'s
    meaning; ``out`` is (F, cost, n_inliers, inlier, best_hyp, best_count, info,
    E): positions 0-6 are what ``init_pairs`` reads, so
    ``init_pairs(store, K, verified)`` works on the result unchanged.
    ``update_flags`` as in ``verify_pairs``."""
    pair_ij, pair_start, index1, index2 = store.pairs(images, min_matches=min_matches)
    x1 = np.column_stack([store.x[index1], store.y[index1]])
    x2 = np.column_stack([store.x[index2], store.y[index2]])
    samples = _core.essential_samples(np.diff(pair_start), H, seed)
    out = _core.essential_pairs(K, pair_start, x1, x2, samples, threshold=threshold, min_inliers=min_inliers)
    order = np.argsort(-out[2].astype(np.int64), kind="stable")
    if update_flags:
        ok = np.repeat(out[6] >= 0, np.diff(pair_start)) & out[3]
        store.flag[index1[ok]] = 1
        store.flag[index2[ok]] = 1
    return order, pair_ij, out, index1, index2


def rematch_verified(keypoints, descriptors, verified, threshold=4.0, min_inliers=15, **match_args):
    """Feed the verified geometry back into matching: match the descriptors of
    every verified pair again, inside a band of ``threshold`` pixels around the
    epipolar lines of its F (``sfm_io.match_descriptors_guided``).  It recovers
    the matches that the unguided ratio test and cross-check lose to repeated
    structure, and so lengthens the tracks.
    ``verified`` is the tuple ``verify_pairs`` / ``verify_pairs_calibrated``
    returned; the pairs with info >= 0 and n_inliers >= ``min_inliers`` are
    taken, in ``verified``'s pair order, with their F from out[0].  In
    ``MatchStore.pairs`` index1 is the observation in pair_ij[p, 0] and index2
    the one in pair_ij[p, 1], and verify_pairs fits x2^T F x1 = 0 to
    x1 = store[index1], x2 = store[index2]: for the pair (i, j) = pair_ij[p]
    that is x_j^T F x_i = 0, the convention of the guided call, so F is passed
    as it is and not transposed.  ``match_args`` (ratio, max_distance,
    cross_check) go to ``match_descriptors_guided``, whose tuple (store,
    pair_ij, match_start, a, b, dsq) is returned; its pair_ij holds the pairs
    taken."""
    _, pair_ij, out = verified[:3]
    keep = (np.asarray(out[6]) >= 0) & (np.asarray(out[2]) >= min_inliers)
    pairs = np.asarray(pair_ij, dtype=np.int64).reshape(-1, 2)[keep]
    F = np.asarray(out[0], dtype=np.float64).reshape(-1, 3, 3)[keep]
    return match_descriptors_guided(keypoints, descriptors, pairs, F, threshold=threshold, **match_args)


def init_pairs(store, K, verified, Hh=128, seed=0, h_threshold=4.0, max_reproj=4.0, min_points=30, min_angle_deg=4.0,
               max_h_ratio=0.8):
    """Which pair to start the reconstruction from, and with what pose and
    points: every verified pair in one device call (``_sfmcore.init_pairs``:
    the pose candidates of its F, cheirality, the winner's points, their
    parallax angles and the support of the best of Hh 4-point homographies).
    The pair of most inliers, ``verify_pairs``'s order[0], is usually the one of
    least baseline, or of a plane: its translation and points are noise.
    ``verified`` is the tuple ``verify_pairs`` returned.  Every pair with verify
    info >= 0 is compacted to its inlier correspondences; the others become
    empty rows.
    Returns (order, eligible, out, pair_start, index1, index2): ``out`` is
    ``_sfmcore.init_pairs``'s tuple over the compacted CSR rows ``pair_start``,
    ``index1`` / ``index2`` the store indices of their observations;
    ``eligible`` (P,) marks the pairs with info == 0, n_good >= min_points,
    median_angle >= min_angle_deg and h_count <= max_h_ratio n_p; ``order``
    puts the eligible pairs first by decreasing n_good (stable), then the rest
    by decreasing n_good.  So pair_ij[order[0]] with out's R, C and the X rows
    where good, together with store.feature[index1], seeds triangulate_store /
    register_views.  The three thresholds are policy defaults to override, not
    measured quantities."""
    _, pair_ij, vout, i1, i2 = verified
    F, inlier, vinfo = vout[0], np.asarray(vout[3], dtype=bool), vout[6]
    P = len(pair_ij)
    n_all = len(i1)
    # the pair of every correspondence: verify_pairs' rows are store.pairs' rows
    if P:
        bounds = _pair_bounds(store, verified)
        per = np.repeat(np.arange(P), np.diff(bounds))
    else:
        per = np.zeros(0, dtype=np.int64)
    keep = inlier & (np.asarray(vinfo)[per] >= 0) if n_all else np.zeros(0, dtype=bool)
    n_p = np.bincount(per[keep], minlength=P).astype(np.int64)
    pair_start = np.concatenate([[0], np.cumsum(n_p)]).astype(np.int64)
    index1, index2 = np.asarray(i1)[keep], np.asarray(i2)[keep]
    x1 = np.column_stack([store.x[index1], store.y[index1]])
    x2 = np.column_stack([store.x[index2], store.y[index2]])
    hs = _core.homography_samples(n_p, Hh, seed) if Hh else None
    out = _core.init_pairs(K, pair_start, x1, x2, F, hs, h_threshold=h_threshold, max_reproj=max_reproj)
    order, eligible = rank_initial_pairs(out, n_p, min_points, min_angle_deg, max_h_ratio)
    return order, eligible, out, pair_start, index1, index2


def pair_rotations(verified, init, min_points=30):
    """The edges of the view graph for ``average_rotations`` from what the chain
    has already computed: ``verified`` is the tuple ``verify_pairs`` /
    ``verify_pairs_calibrated`` returned, ``init`` the tuple ``init_pairs``
    returned for it.  The pairs with init_pairs info == 0 and n_good >=
    ``min_points`` are kept, in ``verified``'s order.
    Returns (pair_ij (E, 2) int32, R_rel (E, 3, 3), weight (E,)): for the pair
    (i, j) init_pairs' camera i is [I | 0] and camera j has R = out[0], so R_rel
    is that R under R_j ~ R_rel R_i; the weight is n_good."""
    pair_ij = np.asarray(verified[1], dtype=np.int32).reshape(-1, 2)
    out = init[2]
    n_good = np.asarray(out[4])
    keep = (np.asarray(out[9]) == 0) & (n_good >= min_points)
    return (np.ascontiguousarray(pair_ij[keep]), np.ascontiguousarray(np.asarray(out[0], dtype=np.float64)[keep]),
            n_good[keep].astype(np.float64))


def average_rotations(pair_ij, R_rel, n_images, weight=None, **args):
    """Every camera's rotation from the pairs' relative rotations in one device
    call (``_sfmcore.average_rotations``, which documents the algorithm, the
    gauge and ``args``: seed, threshold, consensus_sweeps, max_sweeps, tol, and
    refit -- "jacobi", the default, or "cg", the Gauss-Newton refit with the same
    optimum, with rounds, cg_tol, cg_max_iters -- policy defaults to override,
    not measured quantities).  Measured: "cg" reaches ``tol`` in 4 to 5 rounds
    on graphs of up to 300 images; at 10,000 images the default 10 rounds end at
    a step of 7.8e-8, so raise ``rounds`` there and read ``step``.
    Returns (order, out): ``out`` is ``_sfmcore.average_rotations``'s tuple (R,
    edge_angle, edge_inlier, n_inlier_edges, group, info, level, sweeps, and
    with refit="cg" cg_iters, cg_residual, step after them);
    ``order`` lists the images of the largest group first (the lowest label on
    ties), then the other groups by decreasing size, images ascending inside a
    group.  Rotations are consistent inside one group only: R[order[:k]] with k
    the size of the first group is the set to hand on, and edge_inlier says
    which pairs agree with it."""
    out = _core.average_rotations(n_images, pair_ij, R_rel, weight=weight, **args)
    group = np.asarray(out[4], dtype=np.int64)
    size = np.bincount(group, minlength=len(group))[group] if len(group) else group
    order = np.lexsort((np.arange(len(group)), group, -size))
    return order, out


def pair_directions(verified, init, rotations, min_points=30):
    """The edges of the view graph for ``average_positions``: ``verified`` and
    ``init`` as for ``pair_rotations``, ``rotations`` the (order, out) that
    ``average_rotations`` returned for ``pair_rotations(verified, init,
    min_points)``.  Of the pairs ``pair_rotations`` keeps (the same rule, the
    same order), those stay whose ``edge_inlier`` is set and whose two images
    both lie in the first group of ``order``.
    Returns (pair_ij (E, 2) int32, dir (E, 3), weight (E,), keep): ``keep`` (P,)
    bool marks the pairs of ``verified`` taken.  For the pair (i, j) init_pairs'
    camera i is [I | 0] and out[1] is C_rel, the centre of camera j in camera
    i's frame (x_cam = R (X - C)); with the averaged R_i the world direction
    from C_i to C_j is dir = R_i^T C_rel.  The weight is n_good."""
    pair_ij = np.asarray(verified[1], dtype=np.int32).reshape(-1, 2)
    out = init[2]
    n_good = np.asarray(out[4])
    usable = (np.asarray(out[9]) == 0) & (n_good >= min_points)
    order, rot = rotations
    R, inlier, group = np.asarray(rot[0]), np.asarray(rot[2], dtype=bool), np.asarray(rot[4])
    if len(inlier) != int(usable.sum()):
        raise ValueError("pair_directions: rotations do not belong to pair_rotations(verified, init, min_points)")
    in_first = group == group[order[0]] if len(order) else np.zeros(0, dtype=bool)
    keep = usable.copy()
    keep[usable] = inlier & in_first[pair_ij[usable, 0]] & in_first[pair_ij[usable, 1]]
    C_rel = np.asarray(out[1], dtype=np.float64).reshape(-1, 3)[keep]
    dirs = np.einsum("eji,ej->ei", R[pair_ij[keep, 0]], C_rel)
    return np.ascontiguousarray(pair_ij[keep]), np.ascontiguousarray(dirs), n_good[keep].astype(np.float64), keep


def average_positions(pair_ij, dir, n_images, weight=None, **args):
    """Every camera's centre from the pairs' world directions in one device call
    (``_sfmcore.average_positions``, which documents the algorithm and ``args``:
    mu, sigma, threshold, rounds, cg_tol, cg_max_iters, path -- policy defaults
    to override, not measured optima).
    Returns (solved, out): ``out`` is ``_sfmcore.average_positions``'s tuple (C,
    edge_angle, edge_inlier, edge_length, info, cg_iters, cg_residual, n_solved,
    path_used); ``solved`` lists, ascending, the images with info >= 0 -- those
    of the largest component left after leaf pruning, the only ones with a
    centre.  Gauge: the root (info == 1) is at 0 and the weighted mean baseline
    d.(C_j - C_i) is 1, so the scale is arbitrary and the frame is that of the
    rotations the directions were formed with."""
    out = _core.average_positions(n_images, pair_ij, dir, weight=weight, **args)
    return np.flatnonzero(np.asarray(out[4]) >= 0), out


def _pair_bounds(store, verified):
    """the CSR row starts of verify_pairs' correspondences: rows are runs of equal
    (image1, image2) in store.pairs' order, so they follow from the images"""
    _, pair_ij, _, i1, i2 = verified
    key = store.image[np.asarray(i1)].astype(np.int64) * store.n_images + store.image[np.asarray(i2)]
    want = np.asarray(pair_ij, dtype=np.int64).reshape(-1, 2)
    want = want[:, 0] * store.n_images + want[:, 1]
    # every pair has a correspondence and no two pairs share their images
    starts = np.concatenate([[0], np.flatnonzero(np.diff(key)) + 1, [len(key)]]).astype(np.int64)
    if len(starts) != len(want) + 1 or not np.array_equal(key[starts[:-1]], want):
        raise ValueError("init_pairs: `verified` does not belong to this store")
    return starts


def rank_initial_pairs(out, n_p, min_points=30, min_angle_deg=4.0, max_h_ratio=0.8):
    """(order, eligible) of init_pairs' outputs ``out`` over pairs of ``n_p``
    correspondences: eligible where info == 0, n_good >= min_points,
    median_angle >= min_angle_deg and h_count <= max_h_ratio n_p; order puts the
    eligible pairs first by decreasing n_good (stable), then the rest by
    decreasing n_good."""
    n_good, median, h_count, info = out[4], out[5], out[6], out[9]
    n_p = np.asarray(n_p, dtype=np.int64)
    eligible = ((np.asarray(info) == 0) & (np.asarray(n_good) >= min_points)
                & (np.asarray(median) >= np.deg2rad(min_angle_deg))
                & (np.asarray(h_count) <= max_h_ratio * n_p))
    ng = np.asarray(n_good, dtype=np.int64)
    order = np.lexsort((np.arange(len(ng)), -ng, ~eligible))
    return order, eligible


def robust_keep(out, min_inliers, min_angle_deg):
    """The tracks worth keeping among triangulate_tracks_robust's outputs"""
    _, _, n_inliers, _, _, _, info, angle = out
    return (info >= 1) & (n_inliers >= min_inliers) & (angle >= np.deg2rad(min_angle_deg))


def clear_outlier_flags(store, track_start, index, inlier, keep):
    """store.flag = 0 for the observations ``index`` (MatchStore.tracks'
    return_index) that are outliers or belong to a track that is not kept"""
    per_obs_keep = np.repeat(np.asarray(keep, dtype=bool), np.diff(track_start))
    store.flag[index[~(np.asarray(inlier, dtype=bool) & per_obs_keep)]] = 0

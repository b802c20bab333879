"""Matching-file IO (reference Phase 1/Utils.py:8-64).

``get_data`` is a drop-in for the reference's ``Utils.get_data`` (same
signature, same arrays bit for bit) built on the native reader in
libsfmcore (csrc/matching_io.cpp).  ``read_matching`` returns the same data
as a COO ``MatchStore`` -- one record per (feature, image) observation --
so large scenes reach bundle adjustment without the dense
n_features x n_images matrices (800 MB each at cfg5).
"""
import numpy as np

import _sfmcore as _core


class MatchStore:
    """COO observation store: ``feature``, ``image`` (0-based), ``x``, ``y``,
    feature-major with images ascending (the row-major order of the dense
    matrices), plus a per-observation ``flag`` -- the COO form of the
    driver's ``filtered_feature_flags`` (Wrapper_dev.py:98-122)."""

    def __init__(self, n_features, n_images, feature, image, x, y):
        self.n_features = int(n_features)
        self.n_images = int(n_images)
        self.feature, self.image, self.x, self.y = feature, image, x, y
        self.flag = np.zeros(len(feature), dtype=np.uint8)
        self._row_start = np.searchsorted(feature, np.arange(self.n_features + 1))

    def __len__(self):
        return len(self.feature)

    def dense(self):
        """(feature_x, feature_y, feature_flag) exactly as get_data builds them."""
        fx = np.zeros((self.n_features, self.n_images))
        fy = np.zeros((self.n_features, self.n_images))
        ff = np.zeros((self.n_features, self.n_images), dtype=int)
        fx[self.feature, self.image] = self.x
        fy[self.feature, self.image] = self.y
        ff[self.feature, self.image] = 1
        return fx, fy, ff

    def lookup(self, rows, image):
        """Observation index of (rows[i], image), -1 where there is none."""
        rows = np.asarray(rows, dtype=np.int64)
        lo, hi = self._row_start[rows], self._row_start[rows + 1]
        out = np.full(len(rows), -1, dtype=np.int64)
        for k in np.unique(hi - lo):  # rows have few observations: vectorise per length
            sel = (hi - lo) == k
            for j in range(int(k)):
                idx = lo[sel] + j
                hit = self.image[idx] == image
                tgt = np.where(sel)[0][hit]
                out[tgt] = idx[hit]
        return out

    def set_flags(self, rows, image, value=1):
        """filtered_feature_flags[rows, image] = value, for observed entries."""
        idx = self.lookup(rows, image)
        self.flag[idx[idx >= 0]] = value

    def tracks(self, images, use_flags=True, min_views=2, return_index=False):
        """CSR tracks over ``images`` (distinct, ascending image numbers): the
        features with at least ``min_views`` observations among them (flagged
        ones with ``use_flags``), each with all of those observations.
        Returns (feature_rows, track_start, obs_cam, obs_xy): feature_rows
        ascending, track t owning obs_cam / obs_xy[track_start[t]:
        track_start[t + 1]], obs_cam the observation's position in ``images``
        (ascending within a track) -- what np.where on the dense flags'
        columns ``images`` gives, built from the COO rows alone.  With
        ``return_index`` a fifth array follows: the store index of every kept
        observation (into feature / image / x / y / flag), in the tracks'
        order, so that a per-observation result can be written back."""
        images = np.asarray(images, dtype=np.int64).reshape(-1)
        if len(images) and (np.any(np.diff(images) <= 0) or images[0] < 0 or images[-1] >= self.n_images):
            raise ValueError("tracks: images must be distinct, ascending and in [0, n_images)")
        pos = np.full(self.n_images, -1, dtype=np.int32)
        pos[images] = np.arange(len(images), dtype=np.int32)
        keep = pos[self.image] >= 0
        if use_flags:
            keep &= self.flag == 1
        # kept observations per feature row, from the rows' extents
        before = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
        per_row = before[self._row_start[1:]] - before[self._row_start[:-1]]
        feature_rows = np.where(per_row >= max(int(min_views), 1))[0]
        keep &= (per_row >= max(int(min_views), 1))[self.feature]
        track_start = np.concatenate([[0], np.cumsum(per_row[feature_rows], dtype=np.int64)])
        obs_cam = pos[self.image[keep]]
        obs_xy = np.column_stack([self.x[keep], self.y[keep]])
        if return_index:
            return feature_rows, track_start, obs_cam, obs_xy, np.where(keep)[0]
        return feature_rows, track_start, obs_cam, obs_xy

    def correspondences(self, feature_rows, images, use_flags=True):
        """2D-3D correspondences of candidate views: for each image of
        ``images`` (distinct image numbers, any order) its observations whose
        feature is one of ``feature_rows`` (distinct rows: the features that
        have a point) and, with ``use_flags``, whose flag is 1 -- what
        np.where(filtered_world_coords[:, 0] & filtered_feature_flags[:, img])
        selects on the dense matrices (Wrapper_dev.py:232-239), built from the
        COO arrays alone.  Returns view-major CSR (view_start, pt_idx, xy,
        index): view v = images[v] owns [view_start[v], view_start[v + 1]),
        features ascending within it; pt_idx is the feature's position in
        ``feature_rows``, xy the observation, index its place in the store."""
        rows = np.asarray(feature_rows, dtype=np.int64).reshape(-1)
        images = np.asarray(images, dtype=np.int64).reshape(-1)
        if len(images) and (images.min() < 0 or images.max() >= self.n_images
                            or len(np.unique(images)) != len(images)):
            raise ValueError("correspondences: images must be distinct and in [0, n_images)")
        if len(rows) and (rows.min() < 0 or rows.max() >= self.n_features or len(np.unique(rows)) != len(rows)):
            raise ValueError("correspondences: feature_rows must be distinct and in [0, n_features)")
        pos_row = np.full(self.n_features, -1, dtype=np.int64)
        pos_row[rows] = np.arange(len(rows))
        pos_img = np.full(self.n_images, -1, dtype=np.int64)
        pos_img[images] = np.arange(len(images))
        keep = (pos_row[self.feature] >= 0) & (pos_img[self.image] >= 0)
        if use_flags:
            keep &= self.flag == 1
        index = np.where(keep)[0]
        view = pos_img[self.image[index]]
        index = index[np.argsort(view, kind="stable")]  # the store is feature-major: features stay ascending
        view_start = np.concatenate([[0], np.cumsum(np.bincount(view, minlength=len(images)), dtype=np.int64)])
        pt_idx = pos_row[self.feature[index]].astype(np.int32)
        xy = np.column_stack([self.x[index], self.y[index]])
        return view_start.astype(np.int64), pt_idx, xy, index

    def pairs(self, images=None, min_matches=8, use_flags=False):
        """The image pairs of pair verification: for every pair (i, j) of
        ``images`` (distinct image numbers, default all of them) in
        itertools.combinations order that has at least ``min_matches``
        features observed in both (flagged in both with ``use_flags``), its
        correspondences -- what np.where(flag[:, i] & flag[:, j]) selects on
        the dense matrices (Wrapper_dev.py:73-80), built from the COO rows
        alone.  Returns (pair_ij (P, 2) image numbers, pair_start (P + 1,)
        int64, index1, index2): pair p owns [pair_start[p], pair_start[p + 1])
        of index1 / index2, the store indices of the correspondence's
        observation in pair_ij[p, 0] and in pair_ij[p, 1], features ascending
        within a pair."""
        images = np.arange(self.n_images) if images is None else np.asarray(images, dtype=np.int64).reshape(-1)
        n = len(images)
        if n and (images.min() < 0 or images.max() >= self.n_images or len(np.unique(images)) != n):
            raise ValueError("pairs: images must be distinct and in [0, n_images)")
        pos = np.full(self.n_images, -1, dtype=np.int64)
        pos[images] = np.arange(n)
        keep = pos[self.image] >= 0
        if use_flags:
            keep &= self.flag == 1
        kept = np.where(keep)[0]
        # kept observations per feature row, from the rows' extents
        before = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
        lo, m = before[self._row_start[:-1]], np.diff(before[self._row_start])
        o1, o2 = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
        for k in np.unique(m[m >= 2]):  # rows have few observations: vectorise per length
            first = lo[m == k]
            for a in range(int(k) - 1):
                for b in range(a + 1, int(k)):
                    o1.append(kept[first + a])
                    o2.append(kept[first + b])
        o1, o2 = np.concatenate(o1), np.concatenate(o2)
        swap = pos[self.image[o1]] > pos[self.image[o2]]  # the first observation is the earlier of `images`
        o1, o2 = np.where(swap, o2, o1), np.where(swap, o1, o2)
        a, b = pos[self.image[o1]], pos[self.image[o2]]
        pid = a * n - a * (a + 1) // 2 + (b - a - 1)  # the pair's place among the combinations
        per_pair = np.bincount(pid, minlength=n * (n - 1) // 2)
        live = per_pair >= max(int(min_matches), 1)
        sel = live[pid]
        o1, o2, pid = o1[sel], o2[sel], pid[sel]
        order = np.lexsort((self.feature[o1], pid))
        ia, ib = np.triu_indices(n, 1)
        pair_ij = np.column_stack([images[ia[live]], images[ib[live]]]).astype(np.int64).reshape(-1, 2)
        pair_start = np.concatenate([[0], np.cumsum(per_pair[live], dtype=np.int64)]).astype(np.int64)
        return pair_ij, pair_start, o1[order], o2[order]

    def observations(self, filtered_world_coords, n_cameras, use_flags=True):
        """COO inputs of bundle adjustment in the reference's order
        (BundleAdjustment.py:164-169): valid points ascending, cameras
        ascending.  Returns (valid_point_indices, camera_indices,
        point_indices, points_2d) -- the same arrays the dense path gives."""
        valid = np.asarray(filtered_world_coords).flatten() == 1
        valid_point_indices = np.where(valid)[0]
        keep = valid[self.feature] & (self.image < n_cameras)
        if use_flags:
            keep &= self.flag == 1
        feat, cam = self.feature[keep], self.image[keep]
        point_indices = np.searchsorted(valid_point_indices, feat)
        points_2d = np.column_stack([self.x[keep], self.y[keep]])
        return valid_point_indices, cam.astype(np.int64), point_indices, points_2d

    def merge_tracks(self, conflicts="drop"):
        """merge_tracks(self, conflicts): the rows that share a keypoint joined into tracks."""
        return merge_tracks(self, conflicts)


def merge_tracks(store, conflicts="drop"):
    """Join the rows of ``store`` that share a keypoint into tracks, on the
    device (sfm_merge_tracks).  A matching-file line lists only the direct
    matches of one keypoint, so one scene point arrives as several rows; a
    keypoint is an (image, x, y) with equal coordinates, two rows are joined
    when they contain the same keypoint, and a component that holds two
    different keypoints of one image is conflicting: its rows are left out
    (``conflicts="drop"``) or stay the tracks they are (``"keep_rows"``).
    Returns (merged, row_track, obs_map).  ``merged`` is a new MatchStore,
    feature-major with images ascending, which every method and stage accepts
    as it accepts ``store``: its features are the tracks (ascending smallest
    row), its observations the tracks' distinct keypoints with the
    representative's coordinates, its flag the OR of the flags of the store's
    observations that map to it.  ``row_track`` (n_features,) is the merged
    feature of each row of ``store`` or -1, ``obs_map`` (len(store),) the merged
    observation of each of its observations or -1, so that per-row results
    (world points, filtered_world_coords) and per-observation results can be
    carried across.  ``store`` is not modified.  It comes right after
    read_matching and before verify_pairs."""
    policies = {"drop": _core.MERGE_DROP, "keep_rows": _core.MERGE_KEEP_ROWS}
    if conflicts not in policies:
        raise ValueError('merge_tracks: conflicts must be "drop" or "keep_rows"')
    out = _core.merge_tracks(store._row_start, store.image, store.x, store.y, store.n_images, policies[conflicts])
    track_start, track_obs = out["track_start"], out["track_obs"]
    n_tracks = len(out["track_label"])
    feature = np.repeat(np.arange(n_tracks, dtype=np.int32), np.diff(track_start))
    merged = MatchStore(n_tracks, store.n_images, feature, store.image[track_obs].copy(), store.x[track_obs].copy(),
                        store.y[track_obs].copy())
    obs_map = out["obs_slot"].astype(np.int64)
    kept = obs_map >= 0
    np.bitwise_or.at(merged.flag, obs_map[kept], store.flag[kept])
    label = out["label"]
    row_track = np.where(label >= 0, np.searchsorted(out["track_label"], label), -1).astype(np.int64)
    return merged, row_track, obs_map


def match_store(keypoints, pair_ij, match_start, a, b):
    """The MatchStore of a list of matches: one feature row per match, in the
    matches' order, with the two observations (i, keypoints[i][a]) and
    (j, keypoints[j][b]), images ascending inside the row; read_matching's
    dtypes, flags zero."""
    n = len(a)
    per_pair = np.diff(match_start)
    i, j = np.repeat(pair_ij[:, 0], per_pair), np.repeat(pair_ij[:, 1], per_pair)
    image = np.empty((n, 2), dtype=np.int32)
    kp = np.empty((n, 2), dtype=np.int64)
    swap = i > j
    image[:, 0], image[:, 1] = np.where(swap, j, i), np.where(swap, i, j)
    kp[:, 0], kp[:, 1] = np.where(swap, b, a), np.where(swap, a, b)
    start = np.concatenate([[0], np.cumsum([len(k) for k in keypoints])]).astype(np.int64)
    xy = np.concatenate([np.zeros((0, 2))] + [np.asarray(k, dtype=np.float64).reshape(-1, 2) for k in keypoints])
    xy = xy[(start[image] + kp).reshape(-1)]
    feature = np.repeat(np.arange(n, dtype=np.int32), 2)
    return MatchStore(n, len(keypoints), feature, image.reshape(-1), xy[:, 0].copy(), xy[:, 1].copy())


def match_descriptors(keypoints, descriptors, pairs=None, ratio=0.8, max_distance=None, cross_check=True):
    """Match the descriptors of image pairs on the device
    (sfm_match_descriptors) and return the matches as a MatchStore: the stage
    in front of merge_tracks, for images that come with keypoints and
    descriptors of any extractor and not with matching files.
    ``keypoints[k]`` is (N_k, 2) x, y of image k and ``descriptors[k]``
    (N_k, dim) uint8 with dim 64, 128 or 256 (SIFT / RootSIFT as extractors and
    COLMAP store them).  ``pairs`` is (P, 2) image numbers (i, j), i != j, by
    default every itertools.combinations pair.  Keypoint a of i is matched to
    its nearest descriptor b of j (exact integer squared distances, ties to
    the smaller index) when the distance is at most ``max_distance`` (None: no
    limit), the nearest is closer than ``ratio`` times the second nearest
    (squared: d1 < ratio^2 d2) and, with ``cross_check``, a is in turn the
    nearest of b among i's keypoints.  The ratio test is on the direction
    i -> j only, so (i, j) and (j, i) may differ.
    Returns (store, pair_ij, match_start, a, b, dsq): pair p owns
    [match_start[p], match_start[p + 1]) of a, b (keypoint indices local to
    image i and j, ascending a) and dsq (the squared distance); ``store`` has
    one feature row per match in that order with the observations
    (i, keypoints[i][a]) and (j, keypoints[j][b]), images ascending inside the
    row, read_matching's dtypes and zero flags, so store.merge_tracks() joins
    the matches into tracks and verify_pairs accepts either store."""
    kps, desc, img_start, pair_ij, max_dsq = _match_inputs("match_descriptors", keypoints, descriptors, pairs, ratio,
                                                           max_distance)
    out = _core.match_descriptors(desc, img_start, pair_ij, ratio, max_dsq, cross_check)
    store = match_store(kps, pair_ij, out["match_start"], out["a"], out["b"])
    return store, pair_ij, out["match_start"], out["a"], out["b"], out["dsq"]


def match_descriptors_guided(keypoints, descriptors, pairs, F, threshold=4.0, ratio=0.8, max_distance=None,
                             cross_check=True):
    """``match_descriptors`` guided by the pairs' epipolar geometry
    (sfm_match_descriptors_guided): keypoint a of image i is compared only with
    the keypoints of j whose Sampson distance to it under the pair's F is below
    ``threshold`` pixels -- verify_pairs' inlier rule, bit for bit -- and the
    nearest, the second nearest, the ratio test and the cross-check are taken
    over those candidates alone.  Matches that the unguided call loses to
    repeated structure, where two near-identical descriptors in j fail the
    ratio test although only one lies near the epipolar line, come back.
    ``pairs`` (P, 2) is required and ``F`` is (P, 3, 3) with
    x_j^T F x_i = 0 for the pair (i, j), the convention of verify_pairs; a pair
    listed as (j, i) takes F^T.  A pair whose F is not finite (verify_pairs'
    failed pairs) gets no matches.  ``threshold`` must be finite and >= 0.
    Everything else, and the returned (store, pair_ij, match_start, a, b, dsq),
    are ``match_descriptors``'s, so store.merge_tracks() and verify_pairs accept
    the result unchanged."""
    kps, desc, img_start, pair_ij, max_dsq = _match_inputs("match_descriptors_guided", keypoints, descriptors, pairs,
                                                           ratio, max_distance)
    F = np.asarray(F, dtype=np.float64)
    if F.shape != (len(pair_ij), 3, 3):
        raise ValueError("match_descriptors_guided: F must be (P, 3, 3), one matrix per pair")
    if not (np.isfinite(threshold) and threshold >= 0):
        raise ValueError("match_descriptors_guided: threshold must be finite and >= 0")
    xy = np.concatenate([np.zeros((0, 2))] + kps)
    out = _core.match_descriptors_guided(desc, xy, img_start, pair_ij, F, float(threshold), ratio, max_dsq,
                                         cross_check)
    store = match_store(kps, pair_ij, out["match_start"], out["a"], out["b"])
    return store, pair_ij, out["match_start"], out["a"], out["b"], out["dsq"]


def extract_features(images, n_octaves=None, max_keypoints=0, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6,
                     capacity=None):
    """Keypoints and descriptors of greyscale images, on the device
    (sfm_extract_features): the first stage, in front of match_descriptors, for
    images that come without features.  ``images`` is a list or array of 2-D
    uint8 images, all H x W (a caller groups images by size); H, W >= 16.  A
    difference-of-Gaussians detector after Lowe -- octave 0 at the input's size,
    3 layers per octave, ``n_octaves`` octaves (None: as many as keep the
    smaller side >= 16), extrema of |D| above ``contrast_threshold`` refined by
    a quadratic fit and tested against ``edge_threshold`` -- with one keypoint
    per dominant gradient orientation and the 128-byte gradient-histogram
    descriptor that the matcher takes (include/sfmcore.h has every
    definition).  ``sigma`` is the blur of an octave's first layer, in
    (0.5, 3.2].  With ``max_keypoints`` > 0 an image keeps its that many
    largest responses.  The host arrays of a call hold ``capacity`` keypoints
    per image, 172 bytes each: by default max_keypoints, or without a cap
    32,768 (200 images: 1.1 GB); an image with more keypoints raises
    SfmCoreError with its count, and the caller passes a larger ``capacity``
    or a cap.
    Returns (keypoints, descriptors, scale, angle, response), each a list with
    one entry per image: keypoints[k] (N_k, 2) fp64 x, y with pixel centres at
    integers, as in the MatchStore; descriptors[k] (N_k, 128) uint8; scale[k],
    angle[k] (radians in [0, 2 pi), from +x towards +y) and response[k] (N_k,)
    fp32.  An image's keypoints are ordered by (octave, layer, row, column,
    orientation bin) and are the same from run to run.  keypoints and
    descriptors go unchanged into match_descriptors, match_descriptors_guided
    and rematch_verified."""
    name = "extract_features"
    imgs = [np.asarray(im) for im in images]
    for im in imgs:
        if im.dtype != np.uint8 or im.ndim != 2:
            raise ValueError(f"{name}: images[k] must be a 2-D uint8 array")
        if im.shape != imgs[0].shape:
            raise ValueError(f"{name}: the images differ in size; group them by size")
    if n_octaves is not None and (int(n_octaves) != n_octaves or n_octaves < 1):
        raise ValueError(f"{name}: n_octaves must be None or a positive integer")
    if int(max_keypoints) != max_keypoints or max_keypoints < 0:
        raise ValueError(f"{name}: max_keypoints must be an integer >= 0")
    for label, v in (("contrast_threshold", contrast_threshold), ("edge_threshold", edge_threshold)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name}: {label} must be finite and > 0")
    if capacity is not None and (int(capacity) != capacity or capacity < max(int(max_keypoints), 1)):
        raise ValueError(f"{name}: capacity must be a positive integer, at least max_keypoints")
    if not (np.isfinite(sigma) and 0.5 < sigma <= 3.2):
        raise ValueError(f"{name}: sigma must be in (0.5, 3.2]")
    if not imgs:
        return [], [], [], [], []
    H, W = imgs[0].shape
    if H < 16 or W < 16:
        raise ValueError(f"{name}: the images must be at least 16 x 16")
    if n_octaves is not None and n_octaves > _core.extract_octaves(H, W):
        raise ValueError(f"{name}: n_octaves above the {_core.extract_octaves(H, W)} octaves that keep the smaller "
                         "side >= 16")
    out = _core.extract_features(np.stack(imgs), 0 if n_octaves is None else int(n_octaves), int(max_keypoints),
                                 float(contrast_threshold), float(edge_threshold), float(sigma),
                                 capacity=None if capacity is None else int(capacity))
    st = out["kp_start"]
    per_image = [[out[k][st[i]:st[i + 1]].copy() for i in range(len(imgs))]
                 for k in ("xy", "desc", "scale", "angle", "response")]
    return tuple(per_image)


def _retrieval_inputs(name, descriptors):
    """The input checks that the retrieval calls share.  Returns (desc,
    img_start) of the per-image descriptor arrays."""
    descs = [np.asarray(d) for d in descriptors]
    for d in descs:
        if d.dtype != np.uint8 or d.ndim != 2:
            raise ValueError(f"{name}: descriptors[k] must be (N_k, dim) uint8")
        if d.shape[1] != descs[0].shape[1]:
            raise ValueError(f"{name}: the descriptors differ in length")
    if not descs or sum(len(d) for d in descs) == 0:
        raise ValueError(f"{name}: no descriptors")
    if descs[0].shape[1] not in (64, 128, 256):
        raise ValueError(f"{name}: the descriptor length must be 64, 128 or 256")
    desc = np.ascontiguousarray(np.concatenate(descs))
    img_start = np.concatenate([[0], np.cumsum([len(d) for d in descs])]).astype(np.int64)
    return desc, img_start


def _centres_of(name, centres, dim):
    centres = np.asarray(centres)
    if centres.dtype != np.uint8 or centres.ndim != 2 or centres.shape[1] != dim or len(centres) < 1:
        raise ValueError(f"{name}: centres must be (n_words, dim) uint8 with the descriptors' dim")
    return centres


def train_vocabulary(descriptors, n_words, iterations=10, seed=0, max_rows=None):
    """A visual vocabulary of the images' descriptors, on the device
    (sfm_vocab_train): k-means with exact integer arithmetic on
    ``descriptors[k]`` (N_k, dim) uint8, dim 64, 128 or 256.  With ``max_rows``
    below the descriptor count, training uses the deterministic subsample of
    rows floor(k n / max_rows), k = 0 .. max_rows - 1, of the concatenated
    descriptors.  The initial centres are the rows
    np.sort(np.random.default_rng(seed).choice(n, n_words, replace=False)) of
    the training rows; ``n_words`` is clipped to their number.  A descriptor
    belongs to its nearest centre (ties to the smaller index), a centre becomes
    its members' mean rounded half up, an empty cluster keeps its centre, and
    the loop stops after ``iterations`` updates or when nothing changed.
    Returns (centres, report): centres (n_words, dim) uint8 and report a dict
    with word (the training rows' words), count, inertia (one entry per
    assignment, T + 1) and iterations = T.  The result is the same from run to
    run."""
    name = "train_vocabulary"
    desc, _ = _retrieval_inputs(name, descriptors)
    if int(n_words) != n_words or n_words < 1:
        raise ValueError(f"{name}: n_words must be a positive integer")
    if int(iterations) != iterations or iterations < 0:
        raise ValueError(f"{name}: iterations must be an integer >= 0")
    if max_rows is not None:
        if int(max_rows) != max_rows or max_rows < 1:
            raise ValueError(f"{name}: max_rows must be None or a positive integer")
        if max_rows < len(desc):
            desc = np.ascontiguousarray(desc[(np.arange(int(max_rows), dtype=np.int64) * len(desc)) // int(max_rows)])
    n = len(desc)
    n_words = min(int(n_words), n)
    first = np.sort(np.random.default_rng(seed).choice(n, n_words, replace=False))
    out = _core.vocab_train(desc, desc[first], int(iterations))
    return out.pop("centres"), out


def quantize(descriptors, centres):
    """The words of the images' descriptors in a vocabulary, on the device
    (sfm_vocab_train without an update): for every row of ``descriptors[k]``
    the nearest of ``centres`` (n_words, dim) uint8 by exact integer squared
    distance, ties to the smaller index.  Returns a list with one (N_k,) int32
    array per image."""
    desc, img_start = _retrieval_inputs("quantize", descriptors)
    centres = _centres_of("quantize", centres, desc.shape[1])
    if len(centres) > len(desc):
        raise ValueError("quantize: more centres than descriptors")
    word = _core.vocab_train(desc, centres, 0)["word"]
    return [word[img_start[k]:img_start[k + 1]].copy() for k in range(len(img_start) - 1)]


def neighbour_pairs(neighbour):
    """The unique (min(i, j), max(i, j)) over the non-negative entries j of row
    i of ``neighbour``, sorted lexicographically: (P, 2) int32."""
    neighbour = np.asarray(neighbour)
    if neighbour.ndim != 2:
        raise ValueError("neighbour_pairs: neighbour must be (n_images, top_k)")
    i, k = np.nonzero(neighbour >= 0)
    j = neighbour[i, k]
    ij = np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1).reshape(-1, 2)
    return np.unique(ij, axis=0).astype(np.int32).reshape(-1, 2)


def select_pairs(descriptors, centres=None, n_words=4096, top_k=20, iterations=10, seed=0):
    """Choose the image pairs to match by image retrieval, on the device: the
    stage between extract_features and match_descriptors for collections whose
    order says nothing.  The descriptors are quantised against ``centres``
    (default: a vocabulary of ``n_words`` words trained on them by
    train_vocabulary with ``iterations`` and ``seed``; n_words is clipped to the
    number of descriptors), every image becomes a tf-idf vector over the words
    and gets its ``top_k`` most similar images (sfm_select_pairs: integer
    weights floor(256 log(n_images / df) + 0.5), exact int64 dot products, the
    cosine as the score, ties to the smaller image number; an image with fewer
    candidates has its row padded with -1).
    Returns (pairs, neighbour, score, centres): pairs (P, 2) int32, the unique
    (min(i, j), max(i, j)) over all neighbours, sorted -- exactly what
    match_descriptors(pairs=...) takes -- neighbour (n_images, top_k) int32,
    score (n_images, top_k) fp64 and the vocabulary used."""
    name = "select_pairs"
    desc, img_start = _retrieval_inputs(name, descriptors)
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"{name}: top_k must be an integer >= 0")
    if centres is None:
        centres, _ = train_vocabulary(descriptors, n_words, iterations, seed)
    centres = _centres_of(name, centres, desc.shape[1])
    if len(centres) > len(desc):
        raise ValueError(f"{name}: more centres than descriptors")
    word = _core.vocab_train(desc, centres, 0)["word"]
    out = _core.select_pairs(word, img_start, len(centres), int(top_k))
    return neighbour_pairs(out["neighbour"]), out["neighbour"], out["score"], centres


def _match_inputs(name, keypoints, descriptors, pairs, ratio, max_distance):
    """The input checks that the matching calls share.  Returns (keypoints as
    fp64 arrays, desc, img_start, pair_ij, max_dsq)."""
    import itertools
    if len(keypoints) != len(descriptors):
        raise ValueError(f"{name}: keypoints and descriptors need one entry per image")
    n_images = len(keypoints)
    kps, descs = [], []
    for k in range(n_images):
        d = np.asarray(descriptors[k])
        if d.dtype != np.uint8 or d.ndim != 2:
            raise ValueError(f"{name}: descriptors[k] must be (N_k, dim) uint8")
        if descs and d.shape[1] != descs[0].shape[1]:
            raise ValueError(f"{name}: the descriptors differ in length")
        kp = np.asarray(keypoints[k], dtype=np.float64)
        if kp.shape != (len(d), 2):
            raise ValueError(f"{name}: keypoints[k] must be (N_k, 2) with one row per descriptor")
        if not np.isfinite(kp).all():
            raise ValueError(f"{name}: a keypoint coordinate is not finite")
        kps.append(kp)
        descs.append(d)
    if n_images and descs[0].shape[1] not in (64, 128, 256):
        raise ValueError(f"{name}: the descriptor length must be 64, 128 or 256")
    if pairs is None:
        pairs = list(itertools.combinations(range(n_images), 2))
    pair_ij = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pair_ij) and (pair_ij.min() < 0 or pair_ij.max() >= n_images or np.any(pair_ij[:, 0] == pair_ij[:, 1])):
        raise ValueError(f"{name}: pairs must be (i, j) with i != j in [0, n_images)")
    if not (np.isfinite(ratio) and 0.0 < ratio <= 1.0):
        raise ValueError(f"{name}: ratio must be in (0, 1]")
    max_dsq = _core.INT32_MAX
    if max_distance is not None:
        if not (np.isfinite(max_distance) and max_distance >= 0):
            raise ValueError(f"{name}: max_distance must be finite and >= 0")
        max_dsq = int(min(np.floor(float(max_distance) ** 2), _core.INT32_MAX))
    dim = descs[0].shape[1] if n_images else 128
    desc = np.concatenate([np.zeros((0, dim), dtype=np.uint8)] + descs)
    img_start = np.concatenate([[0], np.cumsum([len(d) for d in descs])]).astype(np.int64)
    return kps, desc, img_start, pair_ij, max_dsq


def read_matching(data_path, no_of_images, n_threads=0):
    """Parse data_path/matching1..(no_of_images-1).txt into a MatchStore."""
    nf, feat, img, x, y = _core.parse_matching(data_path, no_of_images, n_threads)
    return MatchStore(nf, no_of_images, feat, img, x, y)


def get_data(data_path, no_of_images):
    """
    Read data from matching files and extract features.

    :param data_path: Path to the directory containing matching files.
    :type data_path: str
    :param no_of_images: Number of images.
    :type no_of_images: int
    :return: x_features, y_features, feature_flags
    :rtype: numpy.ndarray, numpy.ndarray, numpy.ndarray
    """
    return read_matching(data_path, no_of_images).dense()

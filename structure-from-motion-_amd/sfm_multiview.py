"""Multi-view track triangulation from the COO store: one point per feature
from ALL of its views among the registered cameras, in one device call.

The reference's registration loop (Wrapper_dev.py:262-291) triangulates a new
image against every earlier one, a pair at a time, and writes each pair's
points over the last, so a feature seen in five images keeps the point of
two of them.  ``triangulate_store`` differs on purpose: every flagged
observation of a track enters the N-view DLT and the refinement
(``sfm_triangulate_tracks``), with one upload of the observations.
"""
import numpy as np

import _sfmcore as _core
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

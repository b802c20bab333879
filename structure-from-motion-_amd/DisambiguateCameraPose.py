"""Drop-in for the reference module ``DisambiguateCameraPose``
(Phase 1/DisambiguateCameraPose.py:3-93): the cheirality counts of the pose
candidates are taken on the GPU (sfm_cheirality_count), the selection rule and
the two messages are the reference's.
"""
import numpy as np

import _sfmcore as _core


def _counts(Cset, Rset, Xset, live):
    """Cheirality count of each non-empty candidate: candidates with the same
    number of points share a call (at most 8 in one)."""
    counts = {}
    by_len = {}
    for i in live:
        by_len.setdefault(len(Xset[i]), []).append(i)
    for group in by_len.values():
        for k in range(0, len(group), 8):
            ids = group[k:k + 8]
            X = np.stack([np.asarray(Xset[i], dtype=np.float64).reshape(len(Xset[i]), 3) for i in ids])
            c, _ = _core.cheirality_count(np.eye(3), np.zeros(3), Rset[ids], Cset[ids], X)
            counts.update(zip(ids, (int(v) for v in c)))
    return counts


def DisambiguateCameraPose(Cset, Rset, Xset):
    """
    Find unique camera pose by checking the cheirality condition.

    The cheirality condition states that 3D points must be in front of both cameras
    (positive Z coordinate in each camera's coordinate frame).

    Parameters
    ----------
    Cset : array-like
        the set of camera centers (4 x 3 array, each row is a camera center)
    Rset : array-like
        the set of rotation matrices (4 x 3 x 3 array)
    Xset : array-like or list
        set of vectors representing the 3D positions of points in space
        Can be a list of 4 arrays (one for each configuration) or a 4D array
        Each element has shape (N x 3) where N is the number of points

    Results
    -------
    best_C : array-like
        the corrected camera center (3,)
    best_R : array-like
        the corrected rotation matrix (3 x 3)
    best_X : array-like
        the corrected set of vectors representing the 3D positions of points in space (N x 3)
    """
    Cset = np.array(Cset)
    Rset = np.array(Rset)
    Xset = [np.array(Xset[i]) for i in range(len(Xset))]
    # empty candidates are skipped (DisambiguateCameraPose.py:60-61)
    live = [i for i in range(len(Cset)) if len(Xset[i]) > 0]
    if not live:
        print("Warning: No valid camera pose found, using first configuration")
        return Cset[0], Rset[0], Xset[0]
    counts = _counts(Cset, Rset, Xset, live)
    best_idx = live[0]
    for i in live[1:]:
        if counts[i] > counts[best_idx]:  # strict: the earliest maximum wins (:77)
            best_idx = i
    print(f"Selected camera pose configuration {best_idx} with {counts[best_idx]} points in front of both cameras")
    return Cset[best_idx].copy(), Rset[best_idx].copy(), Xset[best_idx].copy()

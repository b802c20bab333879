"""Two-view initialisation in one device call: the step between F-RANSAC and
the first triangulation (Wrapper_dev.py:156-179).

The reference builds E, extracts four pose candidates, triangulates the
inliers under each, counts the points in front of both cameras and
triangulates once more under the winner.  ``two_view_init`` builds E and the
candidates with the two host drop-ins and hands the rest to
``sfm_two_view_select``: one upload of x1 / x2, one launch for the four
triangulations and their counts, and only the winner's points come back.
"""
import numpy as np

import _sfmcore as _core
from EssentialMatrixFromFundamentalMatrix import EssentialMatrixFromFundamentalMatrix
from ExtractCameraPose import ExtractCameraPose


def projection(K, C, R):
    """P = K [R | -R C] as LinearTriangulation.py:44-49 forms it."""
    return K @ np.hstack([R, -R @ C.reshape(3, 1)])


def two_view_init(F, K, x1, x2, return_all=False):
    """Camera 1 at the origin.  Returns (C, R, X, counts, best) -- the selected
    centre and rotation of camera 2, the N x 3 points triangulated under it,
    the candidates' cheirality counts and the selected index (the first
    maximum, as DisambiguateCameraPose) -- and with return_all the candidates'
    points X_all (4, N, 3) as a sixth entry."""
    K = np.array(K)
    x1, x2 = np.array(x1), np.array(x2)
    n = len(x1)
    Cset, Rset = ExtractCameraPose(EssentialMatrixFromFundamentalMatrix(F, K))
    C1, R1 = np.zeros(3), np.eye(3)
    P2s = np.stack([projection(K, C, R) for C, R in zip(Cset, Rset)])
    if n:
        x1, x2 = x1.reshape(n, -1)[:, :2], x2.reshape(n, -1)[:, :2]
    counts, best, X, X_all = _core.two_view_select(projection(K, C1, R1), P2s, R1, C1, Rset, Cset, x1, x2,
                                                   return_all)
    out = (Cset[best].copy(), Rset[best].copy(), X, counts, best)
    return out + (X_all,) if return_all else out

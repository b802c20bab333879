"""Drop-in for the reference module ``ExtractCameraPose``
(Phase 1/ExtractCameraPose.py:3-73): the four (C, R) candidates of an
essential matrix.

This O(1) step stays on the host and on ``np.linalg.svd`` -- the caller's
LAPACK -- on purpose: the ORDER of the four candidates follows the signs LAPACK
gives U and Vt, and on the reference's own data the cheirality counts tie, so
the order decides the selected pose ("Two-view initialisation").
"""
import numpy as np

_W = np.array([[0.0, -1.0, 0.0],
               [1.0, 0.0, 0.0],
               [0.0, 0.0, 1.0]])


def ExtractCameraPose(E):
    """
    Estimate the camera pose given the essential matrix.
    Extracts 4 possible camera pose configurations from the essential matrix.

    Parameters
    ----------
    E : array-like
        The essential matrix (3 x 3)

    Results
    -------
    Cset : array-like
        the set of camera centers (4 x 3 array, each row is a camera center)
    Rset : array-like
        the set of rotation matrices (4 x 3 x 3 array)
    """
    U, _, Vt = np.linalg.svd(np.array(E))
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:  # det(U) det(Vt) = +1
        U[:, -1] *= -1
    t = U[:, 2]
    t = t / np.linalg.norm(t)
    Cset, Rset = [], []
    # (R1, t), (R1, -t), (R2, t), (R2, -t), each with its centre C = -R^T t
    for R in (U @ _W @ Vt, U @ _W.T @ Vt):
        for s in (t, -t):
            Cset.append(-R.T @ s)
            Rset.append(R)
    return np.array(Cset), np.array(Rset)

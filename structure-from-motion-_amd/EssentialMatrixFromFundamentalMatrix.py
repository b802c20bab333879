"""Drop-in for the reference module ``EssentialMatrixFromFundamentalMatrix``
(Phase 1/EssentialMatrixFromFundamentalMatrix.py:3-19): one 3x3 product per
image pair, on the host.
"""
import numpy as np


def EssentialMatrixFromFundamentalMatrix(F, K):
    """
    Computes the essential matrix from the given fundamental matrix and the camera internal matrix.

    Parameters
    ----------
    F : array-like
        The fundamental matrix
    K : array-like
        The camera internal matrix

    Results
    -------
    E : array-like
        The essential matrix
    """
    F, K = np.asarray(F), np.asarray(K)
    return K.T @ F @ K

"""Two-view initialisation, CPU half: the three drop-ins keep the reference's
surface, the host steps (E, the four pose candidates) reproduce
tests/golden/two_view.npz (made by importing the reference,
tests/golden/make_golden_two_view.py), the fixture's counts follow from its
own points, and the device steps fail loudly without a GPU.  The GPU half is
tests/test_two_view_gpu.py.
"""
import inspect
import json
import os

import numpy as np
import pytest

import sfm_synthetic as syn
from conftest import GOLDEN

K = syn.K_REF
GROUPS = ("p3", "syn0", "syn1", "exact")


def load_cases():
    """name -> dict(F, x1, x2, Cset, Rset, X (4, N, 3), counts, sel, line).
    The synthetic pairs are stored once at N = 1025; their smaller sizes are
    prefixes with their own counts, selection and line."""
    g = np.load(os.path.join(GOLDEN, "two_view.npz"))
    cases = {}
    for name in ("p3", "exact"):
        cases[name] = dict(F=g[f"{name}_F"], E=g[f"{name}_E"], x1=g[f"{name}_x1"], x2=g[f"{name}_x2"],
                           Cset=g[f"{name}_Cset"], Rset=g[f"{name}_Rset"], X=g[f"{name}_X"],
                           counts=g[f"{name}_counts"], sel=int(g[f"{name}_sel"]), line=str(g[f"{name}_line"]))
    for seed in (0, 1):
        name = f"syn{seed}"
        x1, x2, _, _ = syn.two_view(seed=seed)
        for k, n in enumerate(g["sizes"]):
            cases[f"{name}_N{n}"] = dict(F=g[f"{name}_F"], E=g[f"{name}_E"], x1=x1[:n], x2=x2[:n],
                                         Cset=g[f"{name}_Cset"], Rset=g[f"{name}_Rset"], X=g[f"{name}_X"][:, :n],
                                         counts=g[f"{name}_counts"][k], sel=int(g[f"{name}_sel"][k]),
                                         line=str(g[f"{name}_line"][k]))
    return cases


CASE_NAMES = ["p3", "exact"] + [f"syn{s}_N{n}" for s in (0, 1) for n in (1, 63, 64, 65, 255, 256, 257, 1025)]


@pytest.fixture(scope="module")
def cases():
    c = load_cases()
    assert sorted(c) == sorted(CASE_NAMES)
    return c


def numpy_counts(Cset, Rset, Xset):
    """The cheirality rule restated (camera 1 at the origin): points with
    positive depth in both cameras per candidate, and the first maximum."""
    counts = np.array([int(np.sum((X[:, 2] > 0) & (((X - C) @ R.T)[:, 2] > 0))) if len(X) else -1
                       for C, R, X in zip(Cset, Rset, Xset)])
    return counts, int(np.argmax(counts))


def blas_config():
    """numpy's BLAS build, as tests/golden/blas_config.json records it"""
    import threadpoolctl
    return [{k: d.get(k) for k in ("internal_api", "version", "architecture", "user_api")}
            for d in threadpoolctl.threadpool_info()
            if d.get("user_api") == "blas" and "numpy" in str(d.get("filepath", ""))]


@pytest.mark.parametrize("mod,sig", [("EssentialMatrixFromFundamentalMatrix", "(F, K)"), ("ExtractCameraPose", "(E)"),
                                     ("DisambiguateCameraPose", "(Cset, Rset, Xset)")])
def test_dropin_signatures(mod, sig):
    m = __import__(mod)
    assert str(inspect.signature(getattr(m, mod))) == sig


def test_two_view_init_signature():
    from sfm_two_view import two_view_init
    assert str(inspect.signature(two_view_init)) == "(F, K, x1, x2, return_all=False)"


@pytest.mark.parametrize("group", GROUPS)
def test_essential_matrix_matches_reference(group):
    from EssentialMatrixFromFundamentalMatrix import EssentialMatrixFromFundamentalMatrix
    g = np.load(os.path.join(GOLDEN, "two_view.npz"))
    E = EssentialMatrixFromFundamentalMatrix(g[f"{group}_F"], K)
    assert np.abs(E - g[f"{group}_E"]).max() <= 1e-12 * np.abs(g[f"{group}_E"]).max()


def _pose_distance(Cset, Rset, Cref, Rref):
    """d[i, j] = largest entry of |pose i - reference pose j| over (C, R)"""
    a = np.concatenate([Cset, Rset.reshape(len(Rset), 9)], axis=1)
    b = np.concatenate([Cref, Rref.reshape(len(Rref), 9)], axis=1)
    return np.abs(a[:, None, :] - b[None, :, :]).max(axis=2)


@pytest.mark.parametrize("group", GROUPS)
def test_extract_camera_pose_set_matches_reference(group):
    """The four poses as a set: the nearest reference pose of each of ours is
    a bijection and every entry agrees to 1e-9 (the set does not depend on
    the signs LAPACK gives U and Vt; the order does)."""
    from ExtractCameraPose import ExtractCameraPose
    g = np.load(os.path.join(GOLDEN, "two_view.npz"))
    Cset, Rset = ExtractCameraPose(g[f"{group}_E"])
    assert Cset.shape == (4, 3) and Rset.shape == (4, 3, 3)
    d = _pose_distance(Cset, Rset, g[f"{group}_Cset"], g[f"{group}_Rset"])
    nearest = d.argmin(axis=1)
    assert sorted(nearest) == [0, 1, 2, 3], (nearest, d)
    assert d[np.arange(4), nearest].max() <= 1e-9, d


@pytest.mark.parametrize("group", GROUPS)
def test_extract_camera_pose_order_matches_reference(group):
    """With the LAPACK the fixtures were made with, the ORDER is the
    reference's too -- the order decides P3Data's 7/7 tie."""
    from ExtractCameraPose import ExtractCameraPose
    pinned = json.load(open(os.path.join(GOLDEN, "blas_config.json")))["numpy_blas"]
    if blas_config() != pinned:
        pytest.skip(f"numpy BLAS {blas_config()} differs from the pinned {pinned}")
    g = np.load(os.path.join(GOLDEN, "two_view.npz"))
    Cset, Rset = ExtractCameraPose(g[f"{group}_E"])
    assert np.abs(Cset - g[f"{group}_Cset"]).max() <= 1e-9
    assert np.abs(Rset - g[f"{group}_Rset"]).max() <= 1e-9


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixture_counts_follow_from_its_points(cases, name):
    c = cases[name]
    counts, sel = numpy_counts(c["Cset"], c["Rset"], c["X"])
    assert np.array_equal(counts, c["counts"]) and sel == c["sel"]
    assert c["line"] == (f"Selected camera pose configuration {sel} with {counts[sel]} points in front of both "
                         "cameras")


def test_p3data_counts_tie():
    g = np.load(os.path.join(GOLDEN, "two_view.npz"))
    assert list(g["p3_counts"]) == [0, 0, 7, 7] and int(g["p3_sel"]) == 2
    assert float(min(g[f"{k}_margin"] for k in GROUPS)) >= 1e-6


def test_device_steps_fail_loudly_without_gpu(cases, monkeypatch):
    """No CPU fallback: with no device visible the counting and the fused
    call raise (the library's device count is patched to 0 so that this also
    holds where a GPU is present)."""
    import _sfmcore
    from DisambiguateCameraPose import DisambiguateCameraPose
    from sfm_two_view import two_view_init
    monkeypatch.setattr(_sfmcore, "_DEVICE_SEEN", False)
    monkeypatch.setattr(_sfmcore._lib, "sfm_device_count", lambda: 0)
    c = cases["p3"]
    with pytest.raises(_sfmcore.SfmCoreError):
        DisambiguateCameraPose(c["Cset"], c["Rset"], list(c["X"]))
    with pytest.raises(_sfmcore.SfmCoreError):
        two_view_init(c["F"], K, c["x1"], c["x2"])
    with pytest.raises(_sfmcore.SfmCoreError):
        _sfmcore.cheirality_count(np.eye(3), np.zeros(3), c["Rset"], c["Cset"], c["X"])

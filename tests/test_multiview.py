"""Multi-view track triangulation, CPU half: MatchStore.tracks against the
dense flags of P3Data, the streamed Givens + Jacobi path restated in numpy
against tests/golden/multiview.npz (made by tests/golden/make_golden_multiview.py),
the C-ABI's argument checks, and the device step failing loudly without a
GPU.  The GPU half is tests/test_multiview_gpu.py; it shares the helpers here.
"""
import os
import re

import numpy as np
import pytest

import sfm_synthetic as syn
from conftest import GOLDEN, REPO

K = syn.K_REF
# name: (n_cams, n_pts, views per point, seed) for sfm_synthetic.ba_problem
# (cfg3's shape: 0.5 px noise); the inputs are regenerated, never stored
CASES = {"v2": (6, 257, 2, 11), "v3": (6, 257, 3, 12), "v5": (7, 257, 5, 13), "v8": (8, 257, 8, 14)}
NVIEW = ("v3", "v5", "v8")


def projection(Kc, C, R):
    """P = K [R | -R C], the expression of sfm_two_view.projection"""
    return Kc @ np.hstack([R, -R @ C.reshape(3, 1)])


def load_problem(name):
    """The tracks of one case: P (n_cams, 3, 4) from the true cameras, CSR
    (track_start, obs_cam, obs_xy), and the cameras themselves."""
    n_cams, n_pts, k, seed = CASES[name]
    p = syn.ba_problem(n_cams, n_pts, k, seed=seed, dense=False)
    P = np.stack([projection(K, C, R) for C, R in zip(p["C_true"], p["R_true"])])
    return dict(P=P, track_start=np.arange(n_pts + 1, dtype=np.int64) * k, obs_cam=p["cam_idx"].astype(np.int32),
                obs_xy=p["obs"], C=p["C_true"], R=p["R_true"], k=k, T=n_pts)


def track(c, t):
    s, e = c["track_start"][t], c["track_start"][t + 1]
    return c["obs_cam"][s:e], c["obs_xy"][s:e]


def dlt_matrix(P, cams, xy):
    """The stacked 2n x 4 system: per view the reference's two rows
    (LinearTriangulation.py:54-90), y p3 - p2 and p1 - x p3."""
    rows = []
    for c, (x, y) in zip(cams, xy):
        rows.append(y * P[c][2] - P[c][1])
        rows.append(P[c][0] - x * P[c][2])
    return np.array(rows)


def dehomogenise(h):
    return h[:3] / h[3] if abs(h[3]) > 1e-8 else h[:3].copy()


def dlt_svd(P, cams, xy):
    """numpy's answer: (X, h, singular values)"""
    _, s, Vt = np.linalg.svd(dlt_matrix(P, cams, xy))
    return dehomogenise(Vt[-1]), Vt[-1], s


def givens_triangle(A):
    """The kernel's streamed QR: each row rotated into a 4 x 4 upper triangle."""
    R = np.zeros((4, 4))
    for row in A:
        a = row.copy()
        for i in range(4):
            if a[i] != 0.0:
                h = np.sqrt(R[i, i] * R[i, i] + a[i] * a[i])
                c, s = R[i, i] / h, a[i] / h
                R[i, i] = h
                for j in range(i + 1, 4):
                    rij, aj = R[i, j], a[j]
                    R[i, j] = c * rij + s * aj
                    a[j] = c * aj - s * rij
    return R


def jacobi_weakest(R, sweeps=40):
    """One-sided Jacobi on the columns of R (sfm_geom.hpp jacobi_onesided) and
    the right singular vector of the column of smallest norm."""
    a, V = R.copy(), np.eye(4)
    for _ in range(sweeps):
        off = 0.0
        for p in range(3):
            for q in range(p + 1, 4):
                al, be, ga = a[:, p] @ a[:, p], a[:, q] @ a[:, q], a[:, p] @ a[:, q]
                r = abs(ga) / np.sqrt(al * be)
                if ga != 0.0 and r > 1e-15:
                    off = max(off, r)
                    zeta = (be - al) / (2.0 * ga)
                    t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                    cs = 1.0 / np.sqrt(1.0 + t * t)
                    sn = cs * t
                    for M in (a, V):
                        x, y = M[:, p].copy(), M[:, q].copy()
                        M[:, p], M[:, q] = cs * x - sn * y, sn * x + cs * y
        if off < 1e-15:
            break
    return V[:, np.argmin((a * a).sum(0))]


def givens_dlt(P, cams, xy):
    return dehomogenise(jacobi_weakest(givens_triangle(dlt_matrix(P, cams, xy))))


def depths(P, cams, X):
    return np.array([P[c][2] @ np.append(X, 1.0) for c in cams])


def residuals(P, cams, xy, X):
    """u - h0/h2, v - h1/h2 per view (NonLinearTriangulation.py:5-50's loss
    over all views); a view with |h2| < 1e-8 contributes zeros."""
    out = []
    for c, (u, v) in zip(cams, xy):
        h = P[c] @ np.append(X, 1.0)
        out += [0.0, 0.0] if abs(h[2]) < 1e-8 else [u - h[0] / h[2], v - h[1] / h[2]]
    return np.array(out)


def cost(P, cams, xy, X):
    r = residuals(P, cams, xy, X)
    return float(r @ r)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "multiview.npz"))


@pytest.fixture(scope="module")
def p3store():
    from sfm_io import read_matching
    return read_matching(os.path.join(GOLDEN, "P3Data"), 5)


def dense_tracks(store, ff, images, min_views=2):
    sub = ff[:, images]
    rows = np.where(sub.sum(1) >= min_views)[0]
    r, c = np.where(sub[rows] == 1)
    fx, fy, _ = store.dense()
    xy = np.column_stack([fx[rows[r], np.asarray(images)[c]], fy[rows[r], np.asarray(images)[c]]])
    start = np.concatenate([[0], np.cumsum(sub[rows].sum(1))])
    return rows, start, c, xy


@pytest.mark.parametrize("images", [[0, 1], [0, 1, 2, 3, 4], [1, 3]])
@pytest.mark.parametrize("flags", ["none", "all", "some"])
def test_tracks_equal_dense_where(p3store, images, flags):
    store = p3store
    rng = np.random.default_rng(5)
    store.flag[:] = {"none": 0, "all": 1, "some": rng.random(len(store)) < 0.6}[flags]
    try:
        ff = np.zeros((store.n_features, store.n_images), dtype=int)
        ff[store.feature, store.image] = store.flag
        for use_flags, dense in ((True, ff), (False, store.dense()[2])):
            rows, start, cam, xy = store.tracks(images, use_flags=use_flags)
            drows, dstart, dcam, dxy = dense_tracks(store, dense, images)
            assert np.array_equal(rows, drows) and np.array_equal(start, dstart)
            assert np.array_equal(cam, dcam) and np.array_equal(xy, dxy)
            assert start.dtype == np.int64 and cam.dtype == np.int32 and xy.shape == (len(cam), 2)
            assert len(start) == len(rows) + 1 and np.all(np.diff(start) >= 2)
        if flags == "none":
            assert len(store.tracks(images)[0]) == 0
    finally:
        store.flag[:] = 0


def test_tracks_histogram_and_min_views(p3store):
    rows, start, cam, _ = p3store.tracks(range(5), use_flags=False)
    n = np.diff(start)
    assert [int((n == k).sum()) for k in (2, 3, 4, 5)] == [2596, 955, 241, 41]
    assert len(rows) == 3833 and int((n >= 3).sum()) == 1237
    rows3, start3, _, _ = p3store.tracks(range(5), use_flags=False, min_views=3)
    assert np.array_equal(rows3, rows[n >= 3]) and np.array_equal(np.diff(start3), n[n >= 3])
    rows1, _, _, _ = p3store.tracks(range(5), use_flags=False, min_views=1)
    assert len(rows1) == p3store.n_features  # every feature has its own image
    with pytest.raises(ValueError):
        p3store.tracks([1, 0])
    with pytest.raises(ValueError):
        p3store.tracks([0, 5])


@pytest.mark.parametrize("name", NVIEW)
def test_streamed_givens_path_agrees_with_fixture(gold, name):
    """The kernel's linear stage restated in numpy (rows streamed through
    Givens rotations into a 4 x 4 triangle, one-sided Jacobi on it) against
    numpy's SVD of the stacked matrix in the fixture, at the GPU test's bound."""
    c = load_problem(name)
    worst = 0.0
    for t in range(c["T"]):
        cams, xy = track(c, t)
        A = dlt_matrix(c["P"], cams, xy)
        R = givens_triangle(A)
        assert np.abs(R.T @ R - A.T @ A).max() <= 1e-12 * np.abs(A.T @ A).max()
        X = dehomogenise(jacobi_weakest(R))
        worst = max(worst, np.abs(X - gold[f"{name}_X_lin"][t]).max())
    assert worst / np.abs(gold[f"{name}_X_lin"]).max() <= 1e-9


def test_fixture_margins(gold):
    for name in CASES:
        assert float(gold[f"{name}_margin"]) >= 1e-6
    for name in NVIEW:
        assert float(gold[f"{name}_cond_eps"]) <= 1e-10
        assert len(gold[f"{name}_X_lin"]) == len(gold[f"{name}_X_min"]) == CASES[name][1]
        assert np.all(gold[f"{name}_cost_min"] <= gold[f"{name}_cost_lin"])


def test_symbol_declared_in_header():
    txt = open(os.path.join(REPO, "include", "sfmcore.h")).read()
    assert re.search(r"\bint sfm_triangulate_tracks\s*\(", txt)
    assert re.search(r"#define SFM_TRACKS_LDS_CAMS \d+", txt)
    import _sfmcore
    assert hasattr(_sfmcore._lib, "sfm_triangulate_tracks") and _sfmcore.version() == 1


def test_bad_arguments_raise():
    import _sfmcore as core
    c = load_problem("v3")
    P, ts, cam, xy = c["P"], c["track_start"][:5], c["obs_cam"][:12], c["obs_xy"][:12]
    bad = {"starts at 0": ts + 1, "decreases": np.array([0, 6, 3, 9, 12]), "end": np.array([0, 3, 6, 9, 11])}
    for what, t in bad.items():
        with pytest.raises(core.SfmCoreError, match="argument: track_start"):
            core.triangulate_tracks(P, t, cam, xy)
    for v in (-1, len(P), 2 ** 31 - 1):
        cb = cam.copy()
        cb[7] = v
        with pytest.raises(core.SfmCoreError, match="argument: camera index"):
            core.triangulate_tracks(P, ts, cb, xy)
    with pytest.raises(core.SfmCoreError, match="argument: refine-only mode needs X0"):
        core.triangulate_tracks(P, ts, cam, xy, refine="only")
    with pytest.raises(core.SfmCoreError, match="argument: max_nfev"):
        core.triangulate_tracks(P, ts, cam, xy, max_nfev=0)
    with pytest.raises(ValueError):
        core.triangulate_tracks(P, ts, cam, xy[:5])
    with pytest.raises(ValueError):
        core.triangulate_tracks(P, ts, cam, xy, X0=np.zeros((3, 3)))
    # the C entry itself, with every output null: rejected before any device work
    rc = core._lib.sfm_triangulate_tracks(core._p(P.reshape(-1, 12)), len(P), core._p(ts + 1, core._i64), 4,
                                          core._p(cam, core._i32), core._p(xy), 12, None, 2, 50, None, None, None,
                                          None, 0)
    assert rc == -1 and b"track_start" in core._lib.sfm_last_error()


def test_no_tracks_returns_empty_without_device(monkeypatch):
    import _sfmcore as core
    monkeypatch.setattr(core, "_DEVICE_SEEN", False)
    monkeypatch.setattr(core._lib, "sfm_device_count", lambda: 0)
    for refine in (False, True):
        X, cst, front, info = core.triangulate_tracks(np.zeros((0, 3, 4)), [0], [], np.zeros((0, 2)), refine=refine)
        assert X.shape == (0, 3) and cst.shape == (0,) and front.shape == (0,) and info.shape == (0,)
        assert front.dtype == bool and info.dtype == np.int32


def test_device_step_fails_loudly_without_gpu(monkeypatch):
    """No CPU fallback: with no device visible the raw call and the store path
    raise (the library's device count is patched to 0 so that this also holds
    where a GPU is present)."""
    import _sfmcore as core
    from sfm_multiview import triangulate_store
    monkeypatch.setattr(core, "_DEVICE_SEEN", False)
    monkeypatch.setattr(core._lib, "sfm_device_count", lambda: 0)
    c = load_problem("v3")
    with pytest.raises(core.SfmCoreError):
        core.triangulate_tracks(c["P"], c["track_start"], c["obs_cam"], c["obs_xy"])
    with pytest.raises(core.SfmCoreError):
        triangulate_store(problem_store(c), K, c["C"], c["R"])


def problem_store(c):
    """The case's observations as a MatchStore with every flag set"""
    from sfm_io import MatchStore
    feat = np.repeat(np.arange(c["T"], dtype=np.int32), c["k"])
    store = MatchStore(c["T"], len(c["P"]), feat, c["obs_cam"], c["obs_xy"][:, 0].copy(), c["obs_xy"][:, 1].copy())
    store.flag[:] = 1
    return store

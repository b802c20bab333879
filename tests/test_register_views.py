"""Batched view registration without a GPU: the store's correspondences, the
sample tables, the argument checks of sfm_register_views (all made on the host
before a device is looked for) and the fixture's own assertions, recomputed.

The scene of tests/golden/register_views.npz is not stored: load_scene
regenerates it from seeds (sfm_synthetic.ba_problem's cameras and points, one
camera per view).  The helpers below are the pieces of the rule in numpy that
the generator (tests/golden/make_golden_register.py) and the GPU tests share.
"""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

import sfm_synthetic as syn

K = syn.K_REF
SEED = 3
SIZES = (5, 6, 7, 63, 64, 65, 257, 1025)
NOISY_FROM = 63          # views of this size and above: 0.5 px noise, and a contaminated twin
HS = (1, 64, 65, 256)
SAMPLE_SEED = 11
OUTLIER_SHARE = 0.3


@functools.lru_cache(maxsize=None)
def load_scene():
    """One batch of views: SIZES clean (5, 6, 7 noise-free, the rest with 0.5 px
    noise), then the views of NOISY_FROM and above again with 30 % of their
    observations displaced by 40-120 px.  View v looks through camera v."""
    sizes = list(SIZES) + [n for n in SIZES if n >= NOISY_FROM]
    V = len(sizes)
    p = syn.ba_problem(V, 1100, 3, seed=SEED, dense=False)
    X = p["X_true"]
    pt, xy, truth = [], [], []
    for v, n in enumerate(sizes):
        rng = np.random.default_rng([SEED, v])
        idx = rng.choice(len(X), n, replace=False)
        h = (K @ (p["R_true"][v] @ (X[idx] - p["C_true"][v]).T)).T
        o = h[:, :2] / h[:, 2:]
        if n >= NOISY_FROM:
            o = o + rng.normal(0, 0.5, o.shape)
        good = np.ones(n, dtype=bool)
        if v >= len(SIZES):
            bad = rng.choice(n, int(round(OUTLIER_SHARE * n)), replace=False)
            ang, mag = rng.uniform(0, 2 * np.pi, len(bad)), rng.uniform(40, 120, len(bad))
            o[bad] += np.column_stack([mag * np.cos(ang), mag * np.sin(ang)])
            good[bad] = False
        pt.append(idx)
        xy.append(o)
        truth.append(good)
    n_v = np.array(sizes, dtype=np.int64)
    return dict(K=K, X=np.ascontiguousarray(X), n_v=n_v, view_start=np.concatenate([[0], np.cumsum(n_v)]),
                pt_idx=np.concatenate(pt).astype(np.int32), xy=np.ascontiguousarray(np.concatenate(xy)),
                truth=np.concatenate(truth), R_true=p["R_true"], C_true=p["C_true"], V=V,
                checked=np.where(n_v >= NOISY_FROM)[0], contaminated=np.arange(V) >= len(SIZES))


def view(sc, v):
    s, e = sc["view_start"][v], sc["view_start"][v + 1]
    return sc["X"][sc["pt_idx"][s:e]], sc["xy"][s:e]


@functools.lru_cache(maxsize=None)
def sample_table(H):
    import _sfmcore
    return _sfmcore.register_samples(load_scene()["n_v"], H, SAMPLE_SEED)


def projection(C, R):
    return K @ np.column_stack([R, -R @ C])


def errors2(P, X, xy):
    """squared reprojection errors and depths under P (3, 4)"""
    h = X @ P[:, :3].T + P[:, 3]
    with np.errstate(all="ignore"):
        d = xy - h[:, :2] / h[:, 2:3]
    return (d * d).sum(axis=1), h[:, 2]


def inlier_mask(P, X, xy, thr):
    e2, h2 = errors2(P, X, xy)
    with np.errstate(invalid="ignore"):
        return (h2 > 0) & ~(np.abs(h2) < 1e-8) & (e2 < thr * thr)


def dlt_rows(Xs, xys):
    """the 2n x 12 system of LinearPnP for n correspondences"""
    xn = (np.linalg.inv(K) @ np.column_stack([xys, np.ones(len(xys))]).T).T
    A = np.zeros((2 * len(Xs), 12))
    for i, (Xw, q) in enumerate(zip(Xs, xn)):
        A[2 * i, :4] = [*Xw, 1.0]
        A[2 * i, 8:] = -q[0] * np.array([*Xw, 1.0])
        A[2 * i + 1, 4:8] = [*Xw, 1.0]
        A[2 * i + 1, 8:] = -q[1] * np.array([*Xw, 1.0])
    return A


def pose_from_null(p):
    """[M | t] = p.reshape(3, 4): M = L R with L lower triangular and a positive
    diagonal after the sign that makes det M > 0, scale = mean(diag L), C =
    -R^T t / scale.  Returns (C, R, P): P = K [M | t] / scale is the projection
    the hypothesis is scored under."""
    M, t = p.reshape(3, 4)[:, :3], p.reshape(3, 4)[:, 3]
    if np.linalg.det(M) < 0:
        M, t = -M, -t
    with np.errstate(all="ignore"):
        l00 = np.linalg.norm(M[0])
        r0 = M[0] / l00
        b = M[1] - (M[1] @ r0) * r0
        l11 = np.linalg.norm(b)
        r1 = b / l11
        r2 = np.cross(r0, r1)
        R = np.array([r0, r1, r2])
        scale = (l00 + l11 + M[2] @ r2) / 3.0
        return -R.T @ (t / scale), R, K @ np.column_stack([M, t]) / scale


def rot_angle(Ra, Rb):
    c = (np.trace(Ra @ Rb.T) - 1.0) / 2.0
    s = np.linalg.norm(Ra @ Rb.T - Rb @ Ra.T) / (2.0 * np.sqrt(2.0))
    return float(np.arctan2(s, c))


# ------------------------------------------------------------------ the store
def random_store(seed, n_features=300, n_images=7):
    from sfm_io import MatchStore
    rng = np.random.default_rng(seed)
    seen = rng.random((n_features, n_images)) < 0.4
    feat, img = np.where(seen)
    st = MatchStore(n_features, n_images, feat.astype(np.int32), img.astype(np.int32),
                    rng.uniform(0, 800, len(feat)), rng.uniform(0, 600, len(feat)))
    st.flag[:] = rng.random(len(feat)) < 0.7
    return st


def dense_correspondences(st, rows, images, use_flags):
    """Wrapper_dev.py:232-239's selection on the dense matrices"""
    fx, fy, ff = st.dense()
    fl = np.zeros((st.n_features, st.n_images), dtype=int)
    fl[st.feature, st.image] = st.flag if use_flags else 1
    has = np.zeros(st.n_features, dtype=int)
    has[rows] = 1
    pos = np.full(st.n_features, -1)
    pos[rows] = np.arange(len(rows))
    vs, pt, xy = [0], [], []
    for im in images:
        idx = np.where(has & fl[:, im] & ff[:, im])[0]
        vs.append(vs[-1] + len(idx))
        pt.append(pos[idx])
        xy.append(np.column_stack([fx[idx, im], fy[idx, im]]))
    return np.array(vs), np.concatenate(pt), np.concatenate(xy).reshape(-1, 2)


def check_correspondences(st, rows, images, use_flags):
    vs, pt, xy, index = st.correspondences(rows, images, use_flags=use_flags)
    dvs, dpt, dxy = dense_correspondences(st, rows, images, use_flags)
    assert vs.dtype == np.int64 and pt.dtype == np.int32
    assert np.array_equal(vs, dvs) and np.array_equal(pt, dpt) and np.array_equal(xy, dxy)
    assert np.array_equal(st.x[index], xy[:, 0]) and np.array_equal(st.y[index], xy[:, 1])
    assert np.array_equal(st.image[index], np.repeat(images, np.diff(vs)))
    assert np.array_equal(st.feature[index], np.asarray(rows)[pt])


@pytest.mark.parametrize("use_flags", [True, False])
def test_correspondences_equal_the_dense_selection_on_a_random_store(use_flags):
    st = random_store(5)
    rng = np.random.default_rng(6)
    rows = np.sort(rng.choice(st.n_features, 120, replace=False))
    check_correspondences(st, rows, np.array([4, 1, 6]), use_flags)
    check_correspondences(st, rng.permutation(rows), np.array([0]), use_flags)  # rows in any order
    check_correspondences(st, rows[:0], np.array([2, 3]), use_flags)


def test_correspondences_equal_the_dense_selection_on_p3data():
    from sfm_io import read_matching
    st = read_matching(os.path.join(GOLDEN, "P3Data"), 5)
    st.flag[:] = np.random.default_rng(0).random(len(st)) < 0.8
    rows = np.where(np.bincount(st.feature[st.image == 0], minlength=st.n_features) > 0)[0]
    check_correspondences(st, rows, np.array([2, 3, 4, 1]), True)
    check_correspondences(st, rows, np.array([2, 3, 4, 1]), False)


def test_correspondences_refuse_bad_arguments():
    st = random_store(5)
    with pytest.raises(ValueError):
        st.correspondences([1, 2], [0, 0])
    with pytest.raises(ValueError):
        st.correspondences([1, 2], [st.n_images])
    with pytest.raises(ValueError):
        st.correspondences([1, 1], [0])


# ------------------------------------------------------------------ samples
def test_register_samples():
    import _sfmcore as core
    counts = [5, 6, 7, 40, 0, 1025]
    t = core.register_samples(counts, 65, 9)
    assert t.shape == (6, 65, 6) and t.dtype == np.int32
    assert not t[0].any() and not t[4].any()          # n_v < 6: zeros
    for v in (1, 2, 3, 5):
        assert t[v].min() >= 0 and t[v].max() < counts[v]
        assert all(len(set(row)) == 6 for row in t[v].tolist())
    assert np.array_equal(t, core.register_samples(counts, 65, 9))          # reproducible by seed
    assert not np.array_equal(t, core.register_samples(counts, 65, 10))
    # a view's table depends on its place and size alone, not on the others
    other = core.register_samples([900, 6, 3, 40], 65, 9)
    assert np.array_equal(other[1], t[1]) and np.array_equal(other[3], t[3])
    with pytest.raises(ValueError):
        core.register_samples(counts, 0, 9)


# ------------------------------------------------------------------ the checks on the host
def small_call():
    sc = load_scene()
    V = 4
    e = int(sc["view_start"][V])
    return dict(K=K, X=sc["X"], view_start=sc["view_start"][:V + 1].copy(), pt_idx=sc["pt_idx"][:e].copy(),
                xy=sc["xy"][:e].copy(), samples=sample_table(64)[:V].copy())


def test_no_views_returns_empty_outputs_without_a_device():
    import _sfmcore as core
    out = core.register_views(K, np.zeros((3, 3)), [0], [], np.zeros((0, 2)), np.zeros((0, 8, 6), dtype=np.int32),
                              want_counts=True, want_models=True)
    C, R, cost, n_inl, inl, hyp, count, info, counts, models = out
    assert C.shape == (0, 3) and R.shape == (0, 3, 3) and inl.shape == (0,) and info.shape == (0,)
    assert counts.shape == (0, 8) and models.shape == (0, 8, 3, 4)


def test_views_of_fewer_than_six_need_no_device():
    import _sfmcore as core
    a = small_call()
    C, R, cost, n_inl, inl, hyp, count, info, counts = core.register_views(
        K, a["X"], a["view_start"][:2], a["pt_idx"][:5], a["xy"][:5], a["samples"][:1], want_counts=True)
    assert info[0] == -1 and not C.any() and np.array_equal(R[0], np.eye(3)) and not inl.any()
    assert n_inl[0] == 0 and hyp[0] == -1 and count[0] == 0 and cost[0] == 0 and not counts.any()


def _edit(a, key, fn):
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    fn(b[key])
    return b


VIOLATIONS = {
    "view_start not from 0": lambda a: _edit(a, "view_start", lambda x: x.__setitem__(0, 1)),
    "view_start decreases": lambda a: _edit(a, "view_start", lambda x: x.__setitem__(2, 3)),
    "view_start ends early": lambda a: _edit(a, "view_start", lambda x: x.__setitem__(-1, x[-1] - 1)),
    "pt_idx negative": lambda a: _edit(a, "pt_idx", lambda x: x.__setitem__(7, -1)),
    "pt_idx past X": lambda a: _edit(a, "pt_idx", lambda x: x.__setitem__(7, 1100)),
    "sample negative": lambda a: _edit(a, "samples", lambda x: x.__setitem__((1, 3, 2), -1)),
    "sample past its view": lambda a: _edit(a, "samples", lambda x: x.__setitem__((1, 3, 2), 6)),
    "sample repeated": lambda a: _edit(a, "samples", lambda x: x.__setitem__((3, 63, 5), x[3, 63, 0])),
}


@pytest.mark.parametrize("name", list(VIOLATIONS))
def test_argument_violations_raise_before_a_device_is_needed(name, monkeypatch):
    import _sfmcore as core

    def no_device():
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(core, "require_device", no_device)
    a = VIOLATIONS[name](small_call())
    with pytest.raises(core.SfmCoreError, match="argument"):
        core.register_views(**a)


@pytest.mark.parametrize("kw", [dict(threshold=0.0), dict(threshold=np.nan), dict(min_inliers=5),
                                dict(refit_rounds=-1), dict(max_nfev=0)])
def test_option_violations_raise_before_a_device_is_needed(kw, monkeypatch):
    import _sfmcore as core
    monkeypatch.setattr(core, "require_device", lambda: (_ for _ in ()).throw(AssertionError("device")))
    with pytest.raises(core.SfmCoreError, match="argument"):
        core.register_views(**small_call(), **kw)


def test_a_bad_sample_in_a_view_of_fewer_than_six_is_ignored():
    import _sfmcore as core
    a = small_call()
    a["samples"][0] = 99
    vs = a["view_start"][:2]
    out = core.register_views(K, a["X"], vs, a["pt_idx"][:5], a["xy"][:5], a["samples"][:1])
    assert out[7][0] == -1


# ------------------------------------------------------------------ the fixture
def test_fixture_assertions_hold_when_recomputed():
    g = np.load(os.path.join(GOLDEN, "register_views.npz"))
    sc = load_scene()
    thr = float(g["threshold"])
    assert np.array_equal(g["truth"], sc["truth"]) and np.array_equal(g["n_v"], sc["n_v"])
    assert set(sc["checked"]) == set(np.where(sc["n_v"] >= 63)[0])  # no view left out
    for v in sc["checked"]:
        X, xy = view(sc, v)
        s, e = sc["view_start"][v], sc["view_start"][v + 1]
        truth = sc["truth"][s:e]
        P = projection(g["C_min"][v], g["R_min"][v])
        e2, h2 = errors2(P, X, xy)
        # the converged minimum on the true inliers separates them from the rest by a pixel
        assert np.array_equal(inlier_mask(P, X, xy, thr), truth)
        assert np.abs(np.sqrt(e2) - thr).min() >= 1.0 and h2.min() > 1.0
        assert np.isclose(e2[truth].sum(), g["cost_min"][v], rtol=1e-9)
        for H in HS[1:]:
            assert g[f"final_margin_H{H}"][v] >= 1.0
            assert np.array_equal(g[f"mask_H{H}"][s:e], truth)

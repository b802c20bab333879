"""Batched initial-pair selection without a GPU: the scene, the whole rule of
sfm_init_pairs restated in numpy (LAPACK's SVD where the device runs Jacobi),
the sample tables, the argument checks (all made on the host before a device is
looked for), the ordering of sfm_multiview.init_pairs and the fixture's own
assertions, recomputed.

The scene of tests/golden/init_pairs.npz is regenerated from seeds; the fixture
holds what the generator (tests/golden/make_golden_init_pairs.py) derived from
the restatement: the F of every pair, the displacements of pair (f) and the
recorded conditions.  Pairs, with K of test_verify_pairs and 0.5 px noise:
  a  a general 3-D scene, baseline 1 at depth 5..12          1000
  b  a's points and 100 more, baseline 1/500 of the depth    1100 (the most)
  c  points of one plane, the wide baseline                   257 (a workgroup + 1)
  d  too few                                                    7
  e0, e1  F all zeros, F with a NaN                        40, 41
  f  pair a, a fifth of x2 moved along its epipolar line     1000
  g  general, the wide baseline                  8, 9, 63, 64, 65
"""
import functools
import os

import numpy as np
import pytest

import test_verify_pairs as vp
from conftest import GOLDEN

import sfm_synthetic as syn

K = vp.K
SEED = 23
NOISE = 0.5
HH = 128
SAMPLE_SEED = 7
H_THRESHOLD = 4.0
MAX_REPROJ = 4.0
MIN_ANGLE_DEG = 4.0
MARGIN = 1e-9
KINDS = ("a", "b", "c", "d", "e0", "e1", "f", "g", "g", "g", "g", "g")
SIZES = (1000, 1100, 257, 7, 40, 41, 1000, 8, 9, 63, 64, 65)
PA, PB, PC, PD, PE0, PE1, PF = 0, 1, 2, 3, 4, 5, 6
R_WIDE = np.array([0.02, -0.15, 0.01])
C_WIDE = np.array([1.0, 0.05, 0.1])
W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


# ------------------------------------------------------------------ the rule in numpy
def candidates(F):
    """the four (R, t) of E = K^T F K, or None (info -2)"""
    E = K.T @ np.asarray(F, dtype=np.float64).reshape(3, 3) @ K
    if not np.all(np.isfinite(E)):
        return None
    U, S, Vt = np.linalg.svd(E)
    if not S[1] > 0:
        return None
    Ra, Rb = U @ W @ Vt, U @ W.T @ Vt
    Ra = -Ra if np.linalg.det(Ra) < 0 else Ra
    Rb = -Rb if np.linalg.det(Rb) < 0 else Rb
    t = U[:, 2]
    return [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]


def proj2(R, t):
    return K @ np.column_stack([R, t])


P1 = K @ np.column_stack([np.eye(3), np.zeros(3)])


def triangulate(P2, x1, x2):
    """the two-view DLT by SVD, dehomogenised where |h3| > 1e-8"""
    A = np.stack([x1[:, 1, None] * P1[2] - P1[1], P1[0] - x1[:, 0, None] * P1[2],
                  x2[:, 1, None] * P2[2] - P2[1], P2[0] - x2[:, 0, None] * P2[2]], axis=1)
    h = np.linalg.svd(A)[2][:, -1]
    big = np.abs(h[:, 3]) > 1e-8
    with np.errstate(all="ignore"):
        return np.where(big[:, None], h[:, :3] / h[:, 3:], h[:, :3])


def depths(R, t, X):
    """(z1, z2) of in_front_of_both and which of them lie within MARGIN, relative, of 0"""
    C = -R.T @ t
    z1, z2 = X[:, 2], (X - C) @ R[2]
    with np.errstate(invalid="ignore"):
        near = (np.abs(z1) <= MARGIN * np.linalg.norm(X, axis=1)) | \
               (np.abs(z2) <= MARGIN * np.linalg.norm(X - C, axis=1))
    return z1, z2, near


def front(R, t, X):
    z1, z2, near = depths(R, t, X)
    with np.errstate(invalid="ignore"):
        return (z1 > 0) & (z2 > 0), near


def reproj2(P, X, x):
    h = np.column_stack([X, np.ones(len(X))]) @ P.T
    with np.errstate(all="ignore"):
        return (x[:, 0] - h[:, 0] / h[:, 2]) ** 2 + (x[:, 1] - h[:, 1] / h[:, 2]) ** 2


def points_under(R, t, x1, x2, max_reproj=MAX_REPROJ):
    """X, good, angle and the correspondences whose decision lies within MARGIN"""
    P2 = proj2(R, t)
    X = triangulate(P2, x1, x2)
    fr, near = front(R, t, X)
    e1, e2 = reproj2(P1, X, x1), reproj2(P2, X, x2)
    m2 = max_reproj ** 2
    with np.errstate(invalid="ignore"):
        good = np.isfinite(X).all(axis=1) & fr & (e1 < m2) & (e2 < m2)
        near = near | (np.abs(e1 - m2) <= 2 * MARGIN * m2) | (np.abs(e2 - m2) <= 2 * MARGIN * m2)
    b = X - (-R.T @ t)
    with np.errstate(invalid="ignore"):
        ang = np.arctan2(np.linalg.norm(np.cross(X, b), axis=1), (X * b).sum(axis=1))
    return X, good, np.where(good, ang, 0.0), near


def lower_median(v):
    n = len(v)
    return 0.0 if n == 0 else float(np.partition(v, (n - 1) // 2)[(n - 1) // 2])


def h_fit(x1, x2):
    """the normalised 4-point DLT under x2 ~ H x1, unit norm and sign"""
    T1, T2 = vp.hartley(x1), vp.hartley(x2)
    (a, b), (c, d) = vp.normalised(T1, x1).T, vp.normalised(T2, x2).T
    z, o = np.zeros(len(a)), np.ones(len(a))
    A = np.stack([np.column_stack([z, z, z, -a, -b, -o, d * a, d * b, d]),
                  np.column_stack([a, b, o, z, z, z, -c * a, -c * b, -c])], axis=1).reshape(-1, 9)
    with np.errstate(all="ignore"):
        return vp.unit_sign(np.linalg.inv(T2) @ np.linalg.svd(A)[2][-1].reshape(3, 3) @ T1), A


def h_transfer2(H, x1, x2):
    """(squared transfer error, h2 usable) per correspondence, for H (..., 3, 3)"""
    h = np.einsum("...ij,nj->...ni", H, np.column_stack([x1, np.ones(len(x1))]))
    with np.errstate(all="ignore"):
        ok = np.isfinite(h[..., 2]) & (np.abs(h[..., 2]) >= 1e-12)
        e = (x2[:, 0] - h[..., 0] / h[..., 2]) ** 2 + (x2[:, 1] - h[..., 1] / h[..., 2]) ** 2
    return e, ok


def h_counts(H, x1, x2, thr):
    e, ok = h_transfer2(H, x1, x2)
    with np.errstate(invalid="ignore"):
        return (ok & (e < thr * thr)).sum(axis=-1)


def first_max(c):
    """the first strictly largest entry"""
    return int(np.argmax(c))


def restate_pair(x1, x2, F, hs, h_thr=H_THRESHOLD, max_reproj=MAX_REPROJ):
    """sfm_init_pairs for one pair: a dict of its outputs"""
    n = len(x1)
    blank = dict(R=np.eye(3), C=np.zeros(3), counts=np.zeros(4, dtype=np.int64), best=0, n_good=0, median=0.0,
                 X=np.zeros((n, 3)), good=np.zeros(n, dtype=bool), angle=np.zeros(n), cands=None,
                 near=np.zeros(n, dtype=bool), h_count=0, h_best=-1, Hbest=np.zeros((3, 3)))
    if n < 8:
        return dict(blank, info=-1)
    out = dict(blank, info=-2)
    if hs is not None and len(hs):
        models = np.array([h_fit(x1[s], x2[s])[0] for s in hs])
        hc = h_counts(models, x1, x2, h_thr)
        out.update(hmodels=models, hcounts=hc)
        if hc.max() > 0:
            b = first_max(hc)
            out.update(h_best=b, h_count=int(hc[b]), Hbest=models[b])
    cands = candidates(F)
    if cands is None:
        return out
    counts, near = np.zeros(4, dtype=np.int64), np.zeros(n, dtype=bool)
    for m, (R, t) in enumerate(cands):
        fr, nr = front(R, t, triangulate(proj2(R, t), x1, x2))
        counts[m] = fr.sum()
        near |= nr
    best = first_max(counts)
    R, t = cands[best]
    X, good, ang, nr = points_under(R, t, x1, x2, max_reproj)
    return dict(out, info=0, cands=cands, counts=counts, best=best, R=R, C=-R.T @ t, X=X, good=good, angle=ang,
                n_good=int(good.sum()), median=lower_median(ang[good]), near=near | nr)


# ------------------------------------------------------------------ the scene
def general_points(rng, n):
    return np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(5, 12, n)])


def observe(rng, X, R2, C2):
    x1 = vp.project(np.eye(3), np.zeros(3), X) + rng.normal(0, NOISE, (len(X), 2))
    x2 = vp.project(R2, C2, X) + rng.normal(0, NOISE, (len(X), 2))
    return x1, x2


def epipolar_direction(F, x1):
    l = np.column_stack([x1, np.ones(len(x1))]) @ np.asarray(F).reshape(3, 3).T
    d = np.column_stack([-l[:, 1], l[:, 0]])
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def raw_pairs():
    """every pair before pair f's displacement: x1, x2, the true (R2, C2)"""
    Rw = syn.rotvec_to_matrix(R_WIDE)[0]
    rng = np.random.default_rng([SEED, 0])
    Xab = general_points(rng, SIZES[PB])
    a = observe(rng, Xab[:SIZES[PA]], Rw, C_WIDE)
    Rb, Cb = syn.rotvec_to_matrix(np.array([0.001, -0.004, 0.002]))[0], np.array([0.017, 0.001, 0.0015])
    b = observe(rng, Xab, Rb, Cb)
    out = []
    for p, (kind, n) in enumerate(zip(KINDS, SIZES)):
        rng = np.random.default_rng([SEED, 1 + p])
        if kind in ("a", "f"):
            out.append((a[0].copy(), a[1].copy(), Rw, C_WIDE))
        elif kind == "b":
            out.append((b[0], b[1], Rb, Cb))
        elif kind == "c":
            xy = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n)])
            X = np.column_stack([xy, 8.0 + 0.3 * xy[:, 0] + 0.2 * xy[:, 1]])
            out.append(observe(rng, X, Rw, C_WIDE) + (Rw, C_WIDE))
        else:
            R2 = syn.rotvec_to_matrix(R_WIDE + rng.normal(0, 0.01, 3))[0]
            C2 = C_WIDE + rng.normal(0, 0.05, 3)
            out.append(observe(rng, general_points(rng, n), R2, C2) + (R2, C2))
    return out


def moved_indices():
    return np.random.default_rng([SEED, 99]).choice(SIZES[PF], SIZES[PF] // 5, replace=False)


def assemble(pairs, F, f_shift):
    """the batch: pair f's x2 displaced by f_shift (px, along its epipolar line under F[PA])"""
    pairs = [list(q) for q in pairs]
    pairs[PF][1] = pairs[PF][1] + f_shift[:, None] * epipolar_direction(F[PA], pairs[PF][0])
    n_p = np.array(SIZES, dtype=np.int64)
    return dict(n_p=n_p, P=len(SIZES), pair_start=np.concatenate([[0], np.cumsum(n_p)]).astype(np.int64),
                x1=np.ascontiguousarray(np.concatenate([q[0] for q in pairs])),
                x2=np.ascontiguousarray(np.concatenate([q[1] for q in pairs])),
                F=np.ascontiguousarray(F), R_true=np.array([q[2] for q in pairs]),
                C_true=np.array([q[3] for q in pairs]), moved=f_shift != 0)


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, "init_pairs.npz"))


@functools.lru_cache(maxsize=None)
def load_scene():
    g = fixture()
    return assemble(raw_pairs(), g["F"], g["f_shift"])


def pair(sc, p):
    s, e = sc["pair_start"][p], sc["pair_start"][p + 1]
    return sc["x1"][s:e], sc["x2"][s:e]


@functools.lru_cache(maxsize=None)
def sample_table(Hh=HH):
    import _sfmcore
    return _sfmcore.homography_samples(load_scene()["n_p"], Hh, SAMPLE_SEED)


@functools.lru_cache(maxsize=None)
def restated(p):
    sc = load_scene()
    x1, x2 = pair(sc, p)
    return restate_pair(x1, x2, sc["F"][p], sample_table()[p])


def pose_errors(R, C, Rt, Ct):
    return vp.rot_angle(R, Rt), vp.direction_angle(C, Ct)


# ------------------------------------------------------------------ the store scene
STORE_SEED = 4


@functools.lru_cache(maxsize=None)
def store_scene():
    """5 images.  Images 0, 1 (baseline 1/500 of the depth) and 2 (wide) see a
    general scene: 160 features in 0 and 1, the first 120 of them in 2 as well.
    Images 3 and 4 (wide) see 100 features of one plane and nothing else."""
    from sfm_io import MatchStore
    rng = np.random.default_rng(STORE_SEED)
    Xg = general_points(rng, 160)
    xy = np.column_stack([rng.uniform(-3, 3, 100), rng.uniform(-2, 2, 100)])
    Xp = np.column_stack([xy, 8.0 + 0.3 * xy[:, 0] + 0.2 * xy[:, 1]])
    Rw = syn.rotvec_to_matrix(R_WIDE)[0]
    R = np.stack([np.eye(3), syn.rotvec_to_matrix(np.array([0.001, -0.004, 0.002]))[0], Rw, np.eye(3), Rw])
    C = np.array([np.zeros(3), [0.017, 0.001, 0.0015], C_WIDE, np.zeros(3), C_WIDE])
    feat, img, xs = [], [], []
    for im, (X, first, count) in enumerate([(Xg, 0, 160), (Xg, 0, 160), (Xg, 0, 120), (Xp, 160, 100), (Xp, 160, 100)]):
        x = vp.project(R[im], C[im], X[:count]) + rng.normal(0, NOISE, (count, 2))
        feat.append(first + np.arange(count)); img.append(np.full(count, im)); xs.append(x)
    feat, img, xs = np.concatenate(feat), np.concatenate(img), np.concatenate(xs)
    o = np.lexsort((img, feat))
    st = MatchStore(260, 5, feat[o].astype(np.int32), img[o].astype(np.int32), np.ascontiguousarray(xs[o, 0]),
                    np.ascontiguousarray(xs[o, 1]))
    return dict(store=st, R=R, C=C)


# ------------------------------------------------------------------ samples
def test_homography_samples():
    import _sfmcore as core
    counts = [3, 4, 5, 40, 0, 1025]
    t = core.homography_samples(counts, 65, 9)
    assert t.shape == (6, 65, 4) and t.dtype == np.int32
    assert not t[0].any() and not t[4].any()          # n_p < 4: zeros
    for p in (1, 2, 3, 5):
        assert t[p].min() >= 0 and t[p].max() < counts[p]
        assert all(len(set(row)) == 4 for row in t[p].tolist())
    assert np.array_equal(t, core.homography_samples(counts, 65, 9))          # reproducible by seed
    assert not np.array_equal(t, core.homography_samples(counts, 65, 10))
    # a pair's table depends on its place and size alone, not on the others
    other = core.homography_samples([900, 4, 2, 40], 65, 9)
    assert np.array_equal(other[1], t[1]) and np.array_equal(other[3], t[3])
    with pytest.raises(ValueError):
        core.homography_samples(counts, 0, 9)


# ------------------------------------------------------------------ the rule
def test_the_restated_candidates_hold_the_true_pose_of_exact_points():
    rng = np.random.default_rng(1)
    Rw = syn.rotvec_to_matrix(R_WIDE)[0]
    X = general_points(rng, 40)
    x1, x2 = vp.project(np.eye(3), np.zeros(3), X), vp.project(Rw, C_WIDE, X)
    r = restate_pair(x1, x2, vp.true_F(Rw, C_WIDE), None)
    assert r["info"] == 0 and r["counts"][r["best"]] == 40 and r["good"].all() and r["h_best"] == -1
    e_rot, e_dir = pose_errors(r["R"], r["C"], Rw, C_WIDE)
    assert e_rot < 1e-9 and e_dir < 1e-9 and abs(np.linalg.norm(r["C"]) - 1) < 1e-12
    scale = np.linalg.norm(C_WIDE)
    assert np.abs(r["X"] * scale - X).max() < 1e-7
    true_angle = np.array([vp.direction_angle(p, p - C_WIDE) for p in X])
    assert np.abs(r["angle"] - true_angle).max() < 1e-9
    assert r["median"] == np.sort(r["angle"])[(40 - 1) // 2]


def test_the_restated_homography_maps_its_sample_and_a_plane():
    rng = np.random.default_rng(2)
    Rw = syn.rotvec_to_matrix(R_WIDE)[0]
    xy = np.column_stack([rng.uniform(-3, 3, 30), rng.uniform(-2, 2, 30)])
    X = np.column_stack([xy, 8.0 + 0.3 * xy[:, 0] + 0.2 * xy[:, 1]])
    x1, x2 = vp.project(np.eye(3), np.zeros(3), X), vp.project(Rw, C_WIDE, X)
    H, _ = h_fit(x1[:4], x2[:4])
    e, ok = h_transfer2(H, x1, x2)
    assert ok.all() and e.max() < 1e-16
    assert abs(np.linalg.norm(H) - 1) < 1e-15 and H.reshape(-1)[np.argmax(np.abs(H))] > 0


# ------------------------------------------------------------------ the checks on the host
def small_call():
    sc = load_scene()
    sel = [PD, 7, 8, 9, 10]   # 7, 8, 9, 63, 64 correspondences
    idx = np.concatenate([np.arange(sc["pair_start"][p], sc["pair_start"][p + 1]) for p in sel])
    return dict(K=K.copy(), pair_start=np.concatenate([[0], np.cumsum(sc["n_p"][sel])]).astype(np.int64),
                x1=sc["x1"][idx].copy(), x2=sc["x2"][idx].copy(), F=sc["F"][sel].copy(),
                hsamples=sample_table(64)[sel].copy())


def no_device(monkeypatch):
    import _sfmcore as core

    def refuse():
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(core, "require_device", refuse)
    return core


def test_no_pairs_returns_empty_outputs_without_a_device(monkeypatch):
    core = no_device(monkeypatch)
    out = core.init_pairs(K, [0], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3, 3)),
                          np.zeros((0, 8, 4), dtype=np.int32), want_cands=True, want_hcounts=True, want_hmodels=True)
    assert len(out) == 16
    assert out[0].shape == (0, 3, 3) and out[2].shape == (0, 4) and out[9].shape == (0,) and out[10].shape == (0, 3)
    assert out[13].shape == (0, 4, 12) and out[14].shape == (0, 8) and out[15].shape == (0, 8, 3, 3)
    assert len(core.init_pairs(K, [0], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3, 3)))) == 13


def test_pairs_of_fewer_than_eight_need_no_device(monkeypatch):
    core = no_device(monkeypatch)
    a = small_call()
    ps = np.array([0, 7, 7, 11])
    hs = core.homography_samples(np.diff(ps), 16, 0)
    R, C, counts, best, n_good, med, h_count, h_best, Hbest, info, X, good, angle, cands, hcounts, hmodels = \
        core.init_pairs(K, ps, a["x1"][:11], a["x2"][:11], a["F"][:3], hs, want_cands=True, want_hcounts=True,
                        want_hmodels=True)
    assert np.all(info == -1) and np.array_equal(R, np.stack([np.eye(3)] * 3)) and not C.any()
    assert not counts.any() and counts.dtype == np.int64 and not best.any() and not n_good.any() and not med.any()
    assert not h_count.any() and np.all(h_best == -1) and not Hbest.any()
    assert X.shape == (11, 3) and not X.any() and not good.any() and good.dtype == bool and not angle.any()
    assert not cands.any() and not hcounts.any() and not hmodels.any()


def _edit(a, key, fn):
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    fn(b[key])
    return b


VIOLATIONS = {
    "pair_start not from 0": lambda a: _edit(a, "pair_start", lambda x: x.__setitem__(0, 1)),
    "pair_start decreases": lambda a: _edit(a, "pair_start", lambda x: x.__setitem__(2, 3)),
    "pair_start ends early": lambda a: _edit(a, "pair_start", lambda x: x.__setitem__(-1, x[-1] - 1)),
    "pair_start ends late": lambda a: _edit(a, "pair_start", lambda x: x.__setitem__(-1, x[-1] + 1)),
    "sample negative": lambda a: _edit(a, "hsamples", lambda x: x.__setitem__((1, 3, 2), -1)),
    "sample past its pair": lambda a: _edit(a, "hsamples", lambda x: x.__setitem__((1, 3, 2), 8)),
    "sample past the last pair": lambda a: _edit(a, "hsamples", lambda x: x.__setitem__((4, 63, 3), 64)),
    "sample repeated": lambda a: _edit(a, "hsamples", lambda x: x.__setitem__((3, 63, 3), x[3, 63, 0])),
    "sample past a pair of seven": lambda a: _edit(a, "hsamples", lambda x: x.__setitem__((0, 5, 1), 7)),
}


@pytest.mark.parametrize("name", list(VIOLATIONS))
def test_argument_violations_raise_before_a_device_is_needed(name, monkeypatch):
    core = no_device(monkeypatch)
    a = VIOLATIONS[name](small_call())
    with pytest.raises(core.SfmCoreError, match="argument"):
        core.init_pairs(**a)


@pytest.mark.parametrize("kw", [dict(h_threshold=0.0), dict(h_threshold=np.nan), dict(h_threshold=np.inf),
                                dict(max_reproj=0.0), dict(max_reproj=-1.0), dict(max_reproj=np.nan),
                                dict(max_reproj=np.inf)])
def test_option_violations_raise_before_a_device_is_needed(kw, monkeypatch):
    core = no_device(monkeypatch)
    with pytest.raises(core.SfmCoreError, match="argument"):
        core.init_pairs(**small_call(), **kw)


def test_a_bad_sample_in_a_pair_of_fewer_than_four_is_ignored(monkeypatch):
    core = no_device(monkeypatch)
    a = small_call()
    hs = np.full((1, 4, 4), 99, dtype=np.int32)
    out = core.init_pairs(K, [0, 3], a["x1"][:3], a["x2"][:3], a["F"][:1], hs)
    assert out[9][0] == -1


def test_wrong_shapes_are_refused():
    import _sfmcore as core
    a = small_call()
    with pytest.raises(ValueError):
        core.init_pairs(**dict(a, x2=a["x2"][:-1]))
    with pytest.raises(ValueError):
        core.init_pairs(**dict(a, hsamples=a["hsamples"][:, :, :3]))
    with pytest.raises(ValueError):
        core.init_pairs(**dict(a, hsamples=a["hsamples"][:4]))
    with pytest.raises(ValueError):
        core.init_pairs(**dict(a, F=a["F"][:4]))
    with pytest.raises(ValueError):
        core.init_pairs(**dict(a, K=np.eye(4)))
    with pytest.raises(ValueError):
        core.init_pairs(**dict(a, pair_start=np.zeros(0, dtype=np.int64)))


# ------------------------------------------------------------------ ordering and eligibility
def hand_made(n_good, median_deg, h_count, info):
    P = len(n_good)
    z = np.zeros(P)
    return (np.zeros((P, 3, 3)), np.zeros((P, 3)), np.zeros((P, 4), dtype=np.int64), z.astype(np.int32),
            np.array(n_good, dtype=np.int32), np.deg2rad(np.array(median_deg, dtype=np.float64)),
            np.array(h_count, dtype=np.int32), z.astype(np.int32), np.zeros((P, 3, 3)),
            np.array(info, dtype=np.int32))


def test_ranking_puts_the_eligible_pairs_first_by_good_points():
    import sfm_multiview as mv
    #                    0     1     2    3    4     5    6     7
    n_p = np.array([1000, 500, 500, 29, 400, 300, 500, 500])
    out = hand_made(n_good=[990, 450, 450, 29, 380, 300, 470, 30],
                    median_deg=[0.2, 6.0, 7.0, 9.0, 8.0, 5.0, 4.0, 4.0],
                    h_count=[1000, 100, 100, 0, 321, 10, 400, 400],
                    info=[0, 0, 0, 0, 0, -2, 0, 0])
    order, eligible = mv.rank_initial_pairs(out, n_p)
    # 0 no parallax, 3 too few points, 4 a plane (321 > 0.8 x 400), 5 no pose; 6 and 7 sit on the limits
    assert eligible.tolist() == [False, True, True, False, False, False, True, True]
    assert order.tolist() == [6, 1, 2, 7, 0, 4, 5, 3]        # ties keep their order
    order, eligible = mv.rank_initial_pairs(out, n_p, min_points=31, min_angle_deg=4.5, max_h_ratio=0.81)
    assert eligible.tolist() == [False, True, True, False, True, False, False, False]
    assert order.tolist() == [1, 2, 4, 0, 6, 5, 7, 3]
    order, eligible = mv.rank_initial_pairs(hand_made([], [], [], []), np.zeros(0))
    assert len(order) == 0 and len(eligible) == 0


def test_init_pairs_compacts_the_verified_inliers(monkeypatch):
    import sfm_multiview as mv
    st = store_scene()["store"]
    pair_ij, ps, i1, i2 = st.pairs()
    P = len(pair_ij)
    assert [tuple(q) for q in pair_ij] == [(0, 1), (0, 2), (1, 2), (3, 4)] and np.diff(ps).tolist() == [160, 120, 120, 100]
    rng = np.random.default_rng(0)
    inlier = rng.random(len(i1)) < 0.8
    vinfo = np.array([1, 2, -3, 0], dtype=np.int32)
    F = rng.normal(size=(P, 3, 3))
    verified = (np.arange(P), pair_ij, (F, np.zeros(P), np.zeros(P, dtype=np.int32), inlier, None, None, vinfo),
                i1, i2)
    seen = {}

    def fake(K_, pair_start, x1, x2, F_, hs, h_threshold, max_reproj):
        seen.update(pair_start=pair_start, x1=x1, x2=x2, F=F_, hs=hs, thr=(h_threshold, max_reproj))
        n_p = np.diff(pair_start)
        return hand_made(n_good=n_p, median_deg=[0.1, 7.0, 6.0, 8.0], h_count=[n_p[0], 5, 0, n_p[3]],
                         info=[0, 0, -1, 0])
    monkeypatch.setattr(mv._core, "init_pairs", fake)
    order, eligible, out, pair_start, index1, index2 = mv.init_pairs(st, K, verified, Hh=32, seed=3, h_threshold=3.0,
                                                                     max_reproj=5.0)
    per = np.repeat(np.arange(P), np.diff(ps))
    keep = inlier & (per != 2)                                # pair 2 has verify info -3: an empty row
    assert np.array_equal(np.diff(pair_start), np.bincount(per[keep], minlength=P)) and pair_start[3] == pair_start[2]
    assert np.array_equal(index1, i1[keep]) and np.array_equal(index2, i2[keep])
    assert np.array_equal(seen["x1"], np.column_stack([st.x[index1], st.y[index1]]))
    assert np.array_equal(seen["x2"], np.column_stack([st.x[index2], st.y[index2]]))
    assert seen["F"] is F and seen["thr"] == (3.0, 5.0)
    import _sfmcore
    assert np.array_equal(seen["hs"], _sfmcore.homography_samples(np.diff(pair_start), 32, 3))
    assert eligible.tolist() == [False, True, False, False] and order[0] == 1
    with pytest.raises(ValueError):
        mv.init_pairs(st, K, (np.arange(P), pair_ij[::-1], verified[2], i1, i2))


# ------------------------------------------------------------------ the fixture
def margin_share(r, n):
    return float(r["near"].sum()) / n


def test_fixture_assertions_hold_when_recomputed():
    g, sc = fixture(), load_scene()
    assert np.array_equal(g["n_p"], sc["n_p"]) and float(g["max_reproj"]) == MAX_REPROJ
    assert float(g["h_threshold"]) == H_THRESHOLD and int(g["Hh"]) == HH
    assert sc["n_p"][PB] == sc["n_p"].max() and (sc["n_p"] == sc["n_p"].max()).sum() == 1
    limit = np.deg2rad(MIN_ANGLE_DEG)
    ra, rb, rc = restated(PA), restated(PB), restated(PC)
    assert rb["median"] < limit < ra["median"]
    assert rc["h_count"] >= 0.95 * sc["n_p"][PC] and ra["h_count"] <= 0.5 * sc["n_p"][PA]
    assert restated(PD)["info"] == -1 and restated(PE0)["info"] == -2 and restated(PE1)["info"] == -2
    assert not sc["F"][PE0].any() and np.isnan(sc["F"][PE1]).sum() == 1
    for p in range(sc["P"]):
        r = restated(p)
        assert r["info"] == g["info"][p]
        if r["info"] != 0:
            continue
        assert margin_share(r, sc["n_p"][p]) < 0.01
        assert np.array_equal(r["counts"], g["counts"][p]) and r["n_good"] == g["n_good"][p]
        assert np.isclose(r["median"], g["median"][p], rtol=1e-9, atol=1e-15)
        e = pose_errors(r["R"], r["C"], sc["R_true"][p], sc["C_true"][p])
        assert np.allclose(e, g["pose_errors"][p], rtol=0, atol=1e-9)
        # the winner stands clear of the other candidates, whichever order they come in
        c = np.sort(r["counts"])
        assert c[3] - c[2] > 0.01 * sc["n_p"][p]
    # pair f: the moved points, and they alone, are not good
    rf = restated(PF)
    assert sc["moved"].sum() == SIZES[PF] // 5 and np.array_equal(rf["good"], ~sc["moved"])
    assert np.array_equal(np.where(sc["moved"])[0], np.sort(moved_indices()))

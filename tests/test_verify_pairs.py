"""Batched pair verification without a GPU: the store's image pairs, the sample
tables, the argument checks of sfm_verify_pairs (all made on the host before a
device is looked for), the rule restated in numpy and the fixture's own
assertions, recomputed.

The scene of tests/golden/verify_pairs.npz is not stored: load_scene
regenerates it from seeds (cfg2's two-view geometry, sfm_synthetic.two_view,
with a small change of pose per pair).  The helpers below are the rule in numpy
that the generator (tests/golden/make_golden_verify_pairs.py) and the GPU tests
share: the fit, the Sampson rule, the winner, the refit rounds and the
not-worse test, with LAPACK's SVD where the device runs Jacobi.
"""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

import sfm_synthetic as syn

K = syn.K_REF
SEED = 5
SIZES = (7, 8, 9, 63, 64, 65, 257, 1025)
NOISY_FROM = 63            # pairs of this size and above carry 0.5 px noise
CONTAMINATED = (64, 65, 257, 1025)   # these appear again with wrong matches
WRONG_SHARE = 0.25
HS = (64, 65, 256)
SAMPLE_SEED = 11
THRESHOLD = 2.5


# ------------------------------------------------------------------ the scene
def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def unit_sign(G):
    """G / |G|_F with the sign that makes the entry of largest magnitude (the
    first such in row-major order) positive"""
    G = np.asarray(G, dtype=np.float64).reshape(3, 3)
    g = G.reshape(-1)
    with np.errstate(all="ignore"):
        k = int(np.argmax(np.abs(g))) if np.all(np.isfinite(g)) else 0
        return G / (-np.linalg.norm(g) if g[k] < 0 else np.linalg.norm(g))


def true_F(R2, C2):
    """x2^T F x1 = 0 for camera 1 at the origin and camera 2 at (R2, C2)"""
    Ki = np.linalg.inv(K)
    return unit_sign(Ki.T @ skew(-R2 @ C2) @ R2 @ Ki)


def project(R, C, X):
    u = (K @ (R @ (X - C).T)).T
    return u[:, :2] / u[:, 2:3]


def displace_along_normal(rng, F, x1_clean, x2, bad):
    """a wrong match: x2 moved by 40-120 px along the normal of its true
    epipolar line, to either side"""
    l = np.column_stack([x1_clean[bad], np.ones(len(bad))]) @ F.T
    nrm = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
    mag = rng.uniform(40, 120, len(bad)) * rng.choice([-1.0, 1.0], len(bad))
    x2[bad] += mag[:, None] * nrm


def make_pair(key, n, noise, wrong_share):
    """cfg2's geometry with a small change of pose drawn from ``key``"""
    rng = np.random.default_rng(key)
    X = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(5, 12, n)])
    R2 = syn.rotvec_to_matrix(np.array([0.02, -0.15, 0.01]) + rng.normal(0, 0.01, 3))[0]
    C2 = np.array([1.0, 0.05, 0.1]) + rng.normal(0, 0.05, 3)
    c1, c2 = project(np.eye(3), np.zeros(3), X), project(R2, C2, X)
    x1, x2 = c1 + rng.normal(0, noise, (n, 2)), c2 + rng.normal(0, noise, (n, 2))
    good = np.ones(n, dtype=bool)
    F = true_F(R2, C2)
    if wrong_share:
        bad = rng.choice(n, int(round(wrong_share * n)), replace=False)
        displace_along_normal(rng, F, c1, x2, bad)
        good[bad] = False
    return x1, x2, good, F, R2, C2


@functools.lru_cache(maxsize=None)
def load_scene():
    """One batch of pairs: SIZES clean (7, 8, 9 noise-free, the rest with 0.5 px
    noise), then CONTAMINATED again with a quarter of their matches wrong."""
    sizes = list(SIZES) + list(CONTAMINATED)
    x1, x2, truth, Ft = [], [], [], []
    for p, n in enumerate(sizes):
        a, b, good, F, _, _ = make_pair([SEED, p], n, 0.5 if n >= NOISY_FROM else 0.0,
                                        WRONG_SHARE if p >= len(SIZES) else 0.0)
        x1.append(a); x2.append(b); truth.append(good); Ft.append(F)
    n_p = np.array(sizes, dtype=np.int64)
    return dict(n_p=n_p, pair_start=np.concatenate([[0], np.cumsum(n_p)]).astype(np.int64),
                x1=np.ascontiguousarray(np.concatenate(x1)), x2=np.ascontiguousarray(np.concatenate(x2)),
                truth=np.concatenate(truth), F_true=np.array(Ft), P=len(sizes),
                checked=np.where(n_p >= 9)[0])


def pair(sc, p):
    s, e = sc["pair_start"][p], sc["pair_start"][p + 1]
    return sc["x1"][s:e], sc["x2"][s:e]


@functools.lru_cache(maxsize=None)
def sample_table(H):
    import _sfmcore
    return _sfmcore.pair_samples(load_scene()["n_p"], H, SAMPLE_SEED)


# ------------------------------------------------------------------ the rule in numpy
def hartley(pts):
    m = pts.mean(axis=0)
    s = np.sqrt(2.0) / (np.sqrt(((pts - m) ** 2).sum(axis=1)).mean() + 1e-8)
    return np.array([[s, 0.0, -s * m[0]], [0.0, s, -s * m[1]], [0.0, 0.0, 1.0]])


def normalised(T, pts):
    return pts * T[0, 0] + T[:2, 2]


def design(x1, x2):
    """rows [c a, c b, c, d a, d b, d, a, b, 1] of the normalised points, with
    the two normalisations"""
    T1, T2 = hartley(x1), hartley(x2)
    (a, b), (c, d) = normalised(T1, x1).T, normalised(T2, x2).T
    return np.column_stack([c * a, c * b, c, d * a, d * b, d, a, b, np.ones(len(a))]), T1, T2


def finish(f, T1, T2):
    """rank 2, F = T2^T F^ T1, unit norm and sign"""
    U, S, Vt = np.linalg.svd(f.reshape(3, 3))
    return unit_sign(T2.T @ (U @ np.diag([S[0], S[1], 0.0]) @ Vt) @ T1)


def fit(x1, x2):
    """the least-squares F of 8 or more correspondences (for 8 the null vector)"""
    A, T1, T2 = design(x1, x2)
    with np.errstate(all="ignore"):
        return finish(np.linalg.svd(A)[2][-1], T1, T2)


def sampson(F, x1, x2):
    """(e^2, den) per correspondence"""
    h1 = np.column_stack([x1, np.ones(len(x1))])
    h2 = np.column_stack([x2, np.ones(len(x2))])
    l, m = h1 @ F.T, h2 @ F
    e = (h2 * l).sum(axis=1)
    return e * e, l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2


def inlier_mask(F, x1, x2, thr):
    e2, den = sampson(F, x1, x2)
    with np.errstate(invalid="ignore"):
        return (den > 0) & (e2 < thr * thr * den)


def distances(F, x1, x2):
    e2, den = sampson(F, x1, x2)
    return np.sqrt(e2 / den)


def cost_of(F, x1, x2, mask):
    e2, den = sampson(F, x1, x2)
    return float((e2[mask] / den[mask]).sum())


def restate_pair(x1, x2, samples, thr, min_inliers=8, rounds=3):
    """sfm_verify_pairs for one pair: a dict of its outputs, and ``models`` /
    ``counts`` of the hypotheses"""
    n = len(x1)
    if n < 8:
        return dict(info=-1, F=np.zeros((3, 3)), mask=np.zeros(n, dtype=bool), best_hyp=-1, best_count=0,
                    cost=0.0)
    models = np.array([fit(x1[s], x2[s]) for s in samples])
    finite = np.isfinite(models).all(axis=(1, 2))
    counts = np.array([int(inlier_mask(F, x1, x2, thr).sum()) if ok else 0 for F, ok in zip(models, finite)])
    out = dict(models=models, counts=counts)
    if not finite.any():
        return dict(out, info=-2, F=np.zeros((3, 3)), mask=np.zeros(n, dtype=bool), best_hyp=-1, best_count=0,
                    cost=0.0)
    h = int(np.argmax(counts)) if counts.max() > 0 else int(np.argmax(finite))
    F, m = models[h], inlier_mask(models[h], x1, x2, thr)
    cost, info = cost_of(F, x1, x2, m), -3
    if counts[h] >= min_inliers:
        info = 2 if rounds else 0
        for _ in range(rounds):
            if m.sum() < 8:
                break
            Fn = fit(x1[m], x2[m])
            m2 = inlier_mask(Fn, x1, x2, thr)
            cost2 = cost_of(Fn, x1, x2, m2)
            if not (m2.sum() > m.sum() or (m2.sum() == m.sum() and cost2 <= cost)):
                break
            changed = not np.array_equal(m, m2)
            F, m, cost = Fn, m2, cost2
            if not changed:
                info = 1
                break
    return dict(out, info=info, F=F, mask=m, best_hyp=h, best_count=int(counts[h]), cost=cost)


def sv_ratio(A):
    """sigma_8 / sigma_1 of a design matrix of 9 columns"""
    s = np.linalg.svd(A, compute_uv=False)
    return s[7] / s[0]


def align(F, G):
    """F with the sign that brings it nearest G"""
    return F if np.abs(F - G).sum() <= np.abs(F + G).sum() else -F


# ------------------------------------------------------------------ the store scene
STORE_SEED = 2
STORE_IMAGES, STORE_FEATURES = 4, 160
STORE_WRONG = {2: 0.25, 3: 0.25}


def rot_angle(Ra, Rb):
    c = (np.trace(Ra @ Rb.T) - 1.0) / 2.0
    s = np.linalg.norm(Ra @ Rb.T - Rb @ Ra.T) / (2.0 * np.sqrt(2.0))
    return float(np.arctan2(s, c))


def direction_angle(a, b):
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


@functools.lru_cache(maxsize=None)
def store_scene():
    """4 images x 160 features, every feature seen in every image, 0.5 px noise;
    a quarter of the observations in images 2 and 3 are wrong matches, moved
    along the normal of their epipolar line against image 0."""
    from sfm_io import MatchStore
    rng = np.random.default_rng(STORE_SEED)
    n, m = STORE_FEATURES, STORE_IMAGES
    X = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(5, 12, n)])
    yaw = np.array([0.0, -0.15, -0.08, 0.1])
    R = syn.rotvec_to_matrix(np.column_stack([rng.normal(0, 0.01, m), yaw, rng.normal(0, 0.01, m)]))
    C = np.column_stack([[0.0, 1.0, 0.5, -0.7], rng.normal(0, 0.05, m), rng.normal(0, 0.05, m)])
    R[0], C[0] = np.eye(3), 0.0
    clean = np.stack([project(R[i], C[i], X) for i in range(m)], axis=1)   # (n, m, 2)
    obs = clean + rng.normal(0, 0.5, clean.shape)
    wrong = np.zeros((n, m), dtype=bool)
    for im, share in STORE_WRONG.items():
        bad = rng.choice(n, int(round(share * n)), replace=False)
        x2 = obs[:, im].copy()
        displace_along_normal(rng, true_F(R[im], C[im]), clean[:, 0], x2, bad)
        obs[:, im] = x2
        wrong[bad, im] = True
    feat = np.repeat(np.arange(n, dtype=np.int32), m)
    img = np.tile(np.arange(m, dtype=np.int32), n)
    st = MatchStore(n, m, feat, img, np.ascontiguousarray(obs[:, :, 0].reshape(-1)),
                    np.ascontiguousarray(obs[:, :, 1].reshape(-1)))
    return dict(store=st, R=R, C=C, wrong=wrong, X=X)


def relative_pose(sc, i, j):
    """camera j in camera i's frame: (R, C)"""
    R = sc["R"][j] @ sc["R"][i].T
    return R, sc["R"][i] @ (sc["C"][j] - sc["C"][i])


# ------------------------------------------------------------------ the store's pairs
def random_store(seed, n_features=300, n_images=6):
    from sfm_io import MatchStore
    rng = np.random.default_rng(seed)
    seen = rng.random((n_features, n_images)) < 0.45
    feat, img = np.where(seen)
    st = MatchStore(n_features, n_images, feat.astype(np.int32), img.astype(np.int32),
                    rng.uniform(0, 800, len(feat)), rng.uniform(0, 600, len(feat)))
    st.flag[:] = rng.random(len(feat)) < 0.7
    return st


def check_pairs(st, images, min_matches, use_flags):
    import itertools
    pair_ij, pair_start, i1, i2 = st.pairs(images, min_matches=min_matches, use_flags=use_flags)
    fl = np.zeros((st.n_features, st.n_images), dtype=int)
    fl[st.feature, st.image] = st.flag if use_flags else 1
    where = np.full((st.n_features, st.n_images), -1)
    where[st.feature, st.image] = np.arange(len(st))
    exp_ij, exp_1, exp_2, exp_start = [], [], [], [0]
    for i, j in itertools.combinations(range(st.n_images) if images is None else images, 2):
        idx = np.where(fl[:, i] & fl[:, j])[0]
        if len(idx) < min_matches:
            continue
        exp_ij.append((i, j))
        exp_1.append(where[idx, i]); exp_2.append(where[idx, j])
        exp_start.append(exp_start[-1] + len(idx))
    assert pair_start.dtype == np.int64
    assert np.array_equal(pair_ij, np.array(exp_ij, dtype=np.int64).reshape(-1, 2))
    assert np.array_equal(pair_start, exp_start)
    assert np.array_equal(i1, np.concatenate(exp_1 + [np.zeros(0, dtype=int)]))
    assert np.array_equal(i2, np.concatenate(exp_2 + [np.zeros(0, dtype=int)]))
    return len(exp_ij)


@pytest.mark.parametrize("use_flags", [False, True])
def test_pairs_equal_the_dense_selection_on_a_random_store(use_flags):
    st = random_store(4)
    assert check_pairs(st, None, 8, use_flags) == 15
    assert check_pairs(st, [4, 1, 5], 8, use_flags) == 3            # images in any order
    median = int(np.median(np.diff(st.pairs(min_matches=1, use_flags=use_flags)[1])))
    assert check_pairs(st, None, median + 1, use_flags) not in (0, 15)   # some pairs fall short
    assert check_pairs(st, [2], 8, use_flags) == 0
    assert check_pairs(st, [], 8, use_flags) == 0


def test_pairs_equal_the_dense_selection_on_p3data():
    from sfm_io import read_matching
    st = read_matching(os.path.join(GOLDEN, "P3Data"), 5)
    assert check_pairs(st, None, 8, False) > 0
    st.flag[:] = np.random.default_rng(0).random(len(st)) < 0.8
    check_pairs(st, None, 8, True)
    check_pairs(st, [3, 0, 2], 30, True)


def test_pairs_refuse_bad_arguments():
    st = random_store(4)
    with pytest.raises(ValueError):
        st.pairs([0, 0])
    with pytest.raises(ValueError):
        st.pairs([st.n_images])


# ------------------------------------------------------------------ samples
def test_pair_samples():
    import _sfmcore as core
    counts = [7, 8, 9, 40, 0, 1025]
    t = core.pair_samples(counts, 65, 9)
    assert t.shape == (6, 65, 8) and t.dtype == np.int32
    assert not t[0].any() and not t[4].any()          # n_p < 8: zeros
    for p in (1, 2, 3, 5):
        assert t[p].min() >= 0 and t[p].max() < counts[p]
        assert all(len(set(row)) == 8 for row in t[p].tolist())
    assert np.array_equal(t, core.pair_samples(counts, 65, 9))          # reproducible by seed
    assert not np.array_equal(t, core.pair_samples(counts, 65, 10))
    # a pair's table depends on its place and size alone, not on the others
    other = core.pair_samples([900, 8, 3, 40], 65, 9)
    assert np.array_equal(other[1], t[1]) and np.array_equal(other[3], t[3])
    with pytest.raises(ValueError):
        core.pair_samples(counts, 0, 9)


def test_register_samples_returns_the_recorded_table():
    import _sfmcore as core
    g = np.load(os.path.join(GOLDEN, "verify_pairs.npz"))
    t = core.register_samples([5, 6, 7, 40, 0, 1025], 65, 9)
    assert t.dtype == np.int32 and np.array_equal(t, g["register_table"])


# ------------------------------------------------------------------ the rule
def test_the_restated_fit_recovers_the_true_matrix_from_exact_points():
    x1, x2, _, F, _, _ = make_pair([1, 2], 8, 0.0, 0.0)
    assert np.abs(align(fit(x1, x2), F) - F).max() < 1e-9
    x1, x2, _, F, _, _ = make_pair([1, 3], 40, 0.0, 0.0)
    G = fit(x1, x2)
    assert np.abs(align(G, F) - F).max() < 1e-9
    assert abs(np.linalg.norm(G) - 1.0) < 1e-15 and G.reshape(-1)[np.argmax(np.abs(G))] > 0
    assert np.linalg.svd(G, compute_uv=False)[2] < 1e-15
    assert distances(G, x1, x2).max() < 1e-9


def test_wrong_matches_lie_far_from_their_epipolar_line():
    sc = load_scene()
    for p in range(len(SIZES), sc["P"]):
        x1, x2 = pair(sc, p)
        s = sc["pair_start"][p]
        good = sc["truth"][s:s + len(x1)]
        d = distances(sc["F_true"][p], x1, x2)
        assert (~good).sum() == int(round(WRONG_SHARE * len(x1)))
        assert d[~good].min() > 25.0 and d[good].max() < THRESHOLD


# ------------------------------------------------------------------ the checks on the host
def small_call():
    sc = load_scene()
    P = 5
    e = int(sc["pair_start"][P])
    return dict(pair_start=sc["pair_start"][:P + 1].copy(), x1=sc["x1"][:e].copy(), x2=sc["x2"][:e].copy(),
                samples=sample_table(64)[:P].copy())


def test_no_pairs_returns_empty_outputs_without_a_device():
    import _sfmcore as core
    out = core.verify_pairs([0], np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 8, 8), dtype=np.int32),
                            want_counts=True, want_models=True)
    F, cost, n_inl, inl, hyp, count, info, counts, models = out
    assert F.shape == (0, 3, 3) and inl.shape == (0,) and info.shape == (0,)
    assert counts.shape == (0, 8) and models.shape == (0, 8, 3, 3)


def test_pairs_of_fewer_than_eight_need_no_device():
    import _sfmcore as core
    a = small_call()
    F, cost, n_inl, inl, hyp, count, info, counts, models = core.verify_pairs(
        a["pair_start"][:2], a["x1"][:7], a["x2"][:7], a["samples"][:1], want_counts=True, want_models=True)
    assert info[0] == -1 and not F.any() and not inl.any() and inl.shape == (7,)
    assert n_inl[0] == 0 and hyp[0] == -1 and count[0] == 0 and cost[0] == 0
    assert not counts.any() and not models.any()


def _edit(a, key, fn):
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    fn(b[key])
    return b


VIOLATIONS = {
    "pair_start not from 0": lambda a: _edit(a, "pair_start", lambda x: x.__setitem__(0, 1)),
    "pair_start decreases": lambda a: _edit(a, "pair_start", lambda x: x.__setitem__(2, 3)),
    "pair_start ends early": lambda a: _edit(a, "pair_start", lambda x: x.__setitem__(-1, x[-1] - 1)),
    "pair_start ends late": lambda a: _edit(a, "pair_start", lambda x: x.__setitem__(-1, x[-1] + 1)),
    "sample negative": lambda a: _edit(a, "samples", lambda x: x.__setitem__((1, 3, 2), -1)),
    "sample past its pair": lambda a: _edit(a, "samples", lambda x: x.__setitem__((1, 3, 2), 8)),
    "sample past the last pair": lambda a: _edit(a, "samples", lambda x: x.__setitem__((4, 63, 7), 64)),
    "sample repeated": lambda a: _edit(a, "samples", lambda x: x.__setitem__((3, 63, 7), x[3, 63, 0])),
}


@pytest.mark.parametrize("name", list(VIOLATIONS))
def test_argument_violations_raise_before_a_device_is_needed(name, monkeypatch):
    import _sfmcore as core

    def no_device():
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(core, "require_device", no_device)
    a = VIOLATIONS[name](small_call())
    with pytest.raises(core.SfmCoreError, match="argument"):
        core.verify_pairs(**a)


@pytest.mark.parametrize("kw", [dict(threshold=0.0), dict(threshold=np.nan), dict(threshold=np.inf),
                                dict(min_inliers=7), dict(refit_rounds=-1)])
def test_option_violations_raise_before_a_device_is_needed(kw, monkeypatch):
    import _sfmcore as core
    monkeypatch.setattr(core, "require_device", lambda: (_ for _ in ()).throw(AssertionError("device")))
    with pytest.raises(core.SfmCoreError, match="argument"):
        core.verify_pairs(**small_call(), **kw)


def test_a_bad_sample_in_a_pair_of_fewer_than_eight_is_ignored():
    import _sfmcore as core
    a = small_call()
    a["samples"][0] = 99
    out = core.verify_pairs(a["pair_start"][:2], a["x1"][:7], a["x2"][:7], a["samples"][:1])
    assert out[6][0] == -1


def test_wrong_shapes_are_refused():
    import _sfmcore as core
    a = small_call()
    with pytest.raises(ValueError):
        core.verify_pairs(a["pair_start"], a["x1"], a["x2"][:-1], a["samples"])
    with pytest.raises(ValueError):
        core.verify_pairs(a["pair_start"], a["x1"], a["x2"], a["samples"][:, :, :6])
    with pytest.raises(ValueError):
        core.verify_pairs(a["pair_start"], a["x1"], a["x2"], a["samples"][:4])


# ------------------------------------------------------------------ the fixture
@functools.lru_cache(maxsize=None)
def restated(p, H):
    sc = load_scene()
    x1, x2 = pair(sc, p)
    return restate_pair(x1, x2, sample_table(H)[p], THRESHOLD)


def test_fixture_assertions_hold_when_recomputed():
    g = np.load(os.path.join(GOLDEN, "verify_pairs.npz"))
    sc = load_scene()
    assert float(g["threshold"]) == THRESHOLD
    assert np.array_equal(g["truth"], sc["truth"]) and np.array_equal(g["n_p"], sc["n_p"])
    assert set(sc["checked"]) == set(np.where(sc["n_p"] >= 9)[0])  # no pair left out
    for p in sc["checked"]:
        x1, x2 = pair(sc, p)
        s, e = sc["pair_start"][p], sc["pair_start"][p + 1]
        truth = sc["truth"][s:e]
        for H in HS:
            F = g[f"F_H{H}"][p]
            # the stored final fit separates the true matches from the wrong ones by half a pixel
            assert np.array_equal(inlier_mask(F, x1, x2, THRESHOLD), truth)
            margin = np.abs(distances(F, x1, x2) - THRESHOLD).min()
            assert margin >= 0.5 and np.isclose(margin, g[f"margin_H{H}"][p], rtol=1e-6)
            assert sv_ratio(design(x1[truth], x2[truth])[0]) >= 1e-4
    # one pair's restatement, recomputed (the generator runs them all)
    p = int(np.where(sc["n_p"] == 65)[0][1])
    r = restated(p, 64)
    assert r["info"] == 1 and np.abs(align(r["F"], g["F_H64"][p]) - g["F_H64"][p]).max() < 1e-12
